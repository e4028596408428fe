// lbm_strain.hip -- what has happened to the packing since a reference state: per grain the displacement, the deformation gradient
// F of its neighbourhood by least squares over the neighbours it had at the reference state, Falk and Langer's D2min (the part of
// the neighbours' motion that F does not explain) and the neighbours it has lost (lbmdem_strain_mark, lbmdem_strain_clear,
// lbmdem_strain_compute, lbmdem_download_strain_grains, lbmdem_strain_grains_device, lbmdem_download_strain_reference,
// lbmdem_write_strain, lbmdem_set_strain_output, lbmdem_write_strain_files; include/lbmdem_hip.h has the contract in full). The mark
// is a copy of the centres, the angles and lbm_structure.hip's list as they are; the compute compares the grains where they are
// now with it: a chain of IEEE double operations in a stated order that one lane walks serially, twice. The census is integers
// and the argmax a reduction over (value, index) pairs; no floating-point atomics anywhere. Nothing here is on the step path: the
// kernels only read the kinematics and the stage's own copy and write to the handle's StrainStage, and nothing is allocated or
// launched before the first mark.
//
// On the handle's stream:
//   k_sn_pack    one lane per grain writes the 32-byte record {X0, Y0, x, y}: a neighbour costs two 16-byte loads out of one
//                aligned record, not four 8-byte loads out of four planes;
//   k_sn_fit     one lane per grain, 64 lanes per workgroup (at 50 000 grains there are 782 wavefronts for 1024 SIMDs: a larger
//                workgroup would only leave CUs idle). The lane walks its segment of the marked list twice, the record of the
//                coming neighbour fetched a round ahead: pass 1 the seven sums, the fit, pass 2 the residual. The census by
//                wavefront sums and one integer atomic per word; the largest D2min by an atomicMax over its key (the bits of a
//                double >= +0.0 order as unsigned integers do);
//   k_sn_arg     one lane per grain: the smallest index among the fitted grains whose key is that maximum, by atomicMin.
// No workgroup waits for another; every loop is bounded by the segment length. LABBOOK.md has the times.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both.
// Front end, as every export's: whole_handle() and SP_REFUSE() (lbmdem_handle.h) for the refusals, MemPool::grow (lbm_mem.h) for
// the scratch kept on the handle, OutFile (lbm_outfile.h) for the files.
#include "lbm_outfile.h"

#include <errno.h>
#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

#ifndef LBMDEM_SINGLE_PRECISION
bool sn_finite(double v) { return v - v == 0.; }

constexpr int SN_LANES = 64;      // grains of a workgroup of the fit: one wavefront
constexpr int SN_THREADS = 256;   // the packing pass and the argmax's second half
// StrainStage::words: the census, then the argmax's two halves
enum : int { SN_FITTED = 0, SN_FEW, SN_DEGENERATE, SN_NONFINITE, SN_ENTRIES, SN_USED, SN_LOST, SN_KEY, SN_ARG, SN_WORDS };

struct SnJob {
  const double *X0, *Y0, *T0;   // the mark
  const double *x, *y, *th;     // the grains where they are now
  const int *off, *nbr;         // the marked list
  long entries;
  int n;
  double rc2;
  double4* rec;                 // [n] {X0, Y0, x, y}
  double *ux, *uy, *drot, *Fxx, *Fxy, *Fyx, *Fyy, *d2min;
  int *used, *lost, *flags;
  unsigned long long* words;
};

__device__ __forceinline__ bool sn_dfinite(double v) { return v - v == 0.; }

__device__ __forceinline__ unsigned long long sn_wave_sum(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}

// the order of the argmax: a double >= +0.0 by its bits; anything else (a NaN; a sum of squares is never negative) counts as +0.0
__device__ __forceinline__ unsigned long long sn_key(double v) {
  return v >= 0. ? (unsigned long long)__double_as_longlong(v) : 0ull;
}

__global__ __launch_bounds__(SN_THREADS) void k_sn_pack(const SnJob J) {
  const int i = blockIdx.x * SN_THREADS + threadIdx.x;
  if (i >= J.n) return;
  J.rec[i] = make_double4(J.X0[i], J.Y0[i], J.x[i], J.y[i]);
}

__global__ __launch_bounds__(SN_LANES) void k_sn_fit(const SnJob J) {
  const int n = J.n;
  const int i = blockIdx.x * SN_LANES + threadIdx.x;
  const bool mine = i < n;
  double ux = 0., uy = 0., drot = 0., Fxx = 0., Fxy = 0., Fyx = 0., Fyy = 0., d2min = 0.;
  int used = 0, lost = 0, flags = 0;
  long entries = 0;
  bool fitted = false;
  if (mine) {
    const double4 me = J.rec[i];
    const double X0 = me.x, Y0 = me.y, xi = me.z, yi = me.w;
    long k0 = J.off[i], k1 = J.off[i + 1];
    if (k0 < 0) k0 = 0;                    // (never: the offsets are a scan of counts)
    if (k1 > J.entries) k1 = J.entries;
    entries = k1 > k0 ? k1 - k0 : 0;
    if (!(sn_dfinite(xi) && sn_dfinite(yi) && sn_dfinite(X0) && sn_dfinite(Y0))) {
      flags = LBMDEM_STRAIN_NONFINITE;
    } else {
      ux = xi - X0; uy = yi - Y0; drot = J.th[i] - J.T0[i];
      // pass 1: the seven sums, the record of the coming neighbour fetched a round ahead
      double Xxx = 0., Xxy = 0., Xyx = 0., Xyy = 0., Yxx = 0., Yxy = 0., Yyy = 0.;
      int jn = -1;
      double4 rn = make_double4(0., 0., 0., 0.);
      if (k0 < k1) {
        jn = J.nbr[k0];
        if (jn >= 0 && jn < n) rn = J.rec[jn];
      }
      for (long k = k0; k < k1; ++k) {
        const int j = jn;
        const double4 rj = rn;
        if (k + 1 < k1) {
          jn = J.nbr[k + 1];
          if (jn >= 0 && jn < n) rn = J.rec[jn];
        }
        if (j < 0 || j >= n) continue;   // (never: the list holds grains)
        const double d0x = rj.x - X0, d0y = rj.y - Y0, dx = rj.z - xi, dy = rj.w - yi;
        if (!(sn_dfinite(dx) && sn_dfinite(dy))) continue;
        ++used;
        if (dx * dx + dy * dy > J.rc2) ++lost;
        Xxx += dx * d0x; Xxy += dx * d0y; Xyx += dy * d0x; Xyy += dy * d0y;
        Yxx += d0x * d0x; Yxy += d0x * d0y; Yyy += d0y * d0y;
      }
      const double det = Yxx * Yyy - Yxy * Yxy;
      if (used < 2) flags = LBMDEM_STRAIN_FEW;
      else if (!(det > 0x1p-40 * (Yxx * Yyy))) flags = LBMDEM_STRAIN_DEGENERATE;
      if (!flags) {
        fitted = true;
        const double Ixx = Yyy / det, Ixy = (-Yxy) / det, Iyy = Yxx / det;
        Fxx = Xxx * Ixx + Xxy * Ixy; Fxy = Xxx * Ixy + Xxy * Iyy;
        Fyx = Xyx * Ixx + Xyy * Ixy; Fyy = Xyx * Ixy + Xyy * Iyy;
        // pass 2: the residual over the same neighbours
        if (k0 < k1) {
          jn = J.nbr[k0];
          if (jn >= 0 && jn < n) rn = J.rec[jn];
        }
        for (long k = k0; k < k1; ++k) {
          const int j = jn;
          const double4 rj = rn;
          if (k + 1 < k1) {
            jn = J.nbr[k + 1];
            if (jn >= 0 && jn < n) rn = J.rec[jn];
          }
          if (j < 0 || j >= n) continue;
          const double d0x = rj.x - X0, d0y = rj.y - Y0, dx = rj.z - xi, dy = rj.w - yi;
          if (!(sn_dfinite(dx) && sn_dfinite(dy))) continue;
          const double rx = dx - (Fxx * d0x + Fxy * d0y), ry = dy - (Fyx * d0x + Fyy * d0y);
          d2min += rx * rx + ry * ry;
        }
      }
    }
    J.ux[i] = ux; J.uy[i] = uy; J.drot[i] = drot;
    J.Fxx[i] = Fxx; J.Fxy[i] = Fxy; J.Fyx[i] = Fyx; J.Fyy[i] = Fyy; J.d2min[i] = d2min;
    J.used[i] = used; J.lost[i] = lost; J.flags[i] = flags;
  }
  // the census: sums of the wavefront, then one integer atomic per word
  const unsigned long long c_fit = sn_wave_sum(fitted ? 1ull : 0ull);
  const unsigned long long c_few = sn_wave_sum((flags & LBMDEM_STRAIN_FEW) ? 1ull : 0ull);
  const unsigned long long c_deg = sn_wave_sum((flags & LBMDEM_STRAIN_DEGENERATE) ? 1ull : 0ull);
  const unsigned long long c_bad = sn_wave_sum((flags & LBMDEM_STRAIN_NONFINITE) ? 1ull : 0ull);
  const unsigned long long c_ent = sn_wave_sum((unsigned long long)entries);
  const unsigned long long c_used = sn_wave_sum((unsigned long long)used);
  const unsigned long long c_lost = sn_wave_sum((unsigned long long)lost);
  unsigned long long c_key = fitted ? sn_key(d2min) : 0ull;
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(c_key, s);
    c_key = o > c_key ? o : c_key;
  }
  if (threadIdx.x == 0) {
    if (c_fit) atomicAdd(&J.words[SN_FITTED], c_fit);
    if (c_few) atomicAdd(&J.words[SN_FEW], c_few);
    if (c_deg) atomicAdd(&J.words[SN_DEGENERATE], c_deg);
    if (c_bad) atomicAdd(&J.words[SN_NONFINITE], c_bad);
    if (c_ent) atomicAdd(&J.words[SN_ENTRIES], c_ent);
    if (c_used) atomicAdd(&J.words[SN_USED], c_used);
    if (c_lost) atomicAdd(&J.words[SN_LOST], c_lost);
    if (c_key) atomicMax(&J.words[SN_KEY], c_key);
  }
}

// (behind k_sn_fit on the stream: words[SN_KEY] is final; words[SN_ARG] starts as all ones)
__global__ __launch_bounds__(SN_THREADS) void k_sn_arg(const SnJob J) {
  const int i = blockIdx.x * SN_THREADS + threadIdx.x;
  if (i >= J.n) return;
  if (J.flags[i] == 0 && sn_key(J.d2min[i]) == J.words[SN_KEY]) atomicMin(&J.words[SN_ARG], (unsigned long long)i);
}

int sn_blocks(long items, int threads) { return (int)((items + threads - 1) / threads); }

int strain_marked(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  if (!h->sn.marked) return fail(LBMDEM_EINVAL, "%s: no lbmdem_strain_mark has been made on this handle", who);
  return LBMDEM_OK;
}

int strain_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  const auto& T = h->sn;
  if (!T.marked || !T.valid || T.of_mark != T.mark_gen || T.seq != h->substep_seq || T.moved != h->grains_moved)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_strain_compute has been made for the mark and the grains where they are now", who);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_strain_files(const char* dir, int nfile, int n, const double* ux, const double* uy, const double* drot,
                              const double* Fxx, const double* Fxy, const double* Fyx, const double* Fyy, const double* d2min,
                              const int* used, const int* lost, const int* flags, double rc2, const long* counts8, double t,
                              double t_mark) try {
  if (n < 1 || !ux || !uy || !drot || !Fxx || !Fxy || !Fyx || !Fyy || !d2min || !used || !lost || !flags || !counts8)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_strain_files arguments");
  for (int i = 0; i < n; ++i) {
    if (used[i] < 0 || used[i] >= n || lost[i] < 0 || lost[i] > used[i])
      return fail(LBMDEM_EINVAL, "lbmdem_write_strain_files: grain %d has lost %d of %d neighbours used, of %d grains", i, lost[i],
                  used[i], n);
    if (flags[i] < 0 || flags[i] > 7)
      return fail(LBMDEM_EINVAL, "lbmdem_write_strain_files: grain %d has flags %d, outside 0 .. 7", i, flags[i]);
  }
  OutFile F;
  RC_TRY(F.open("w", dir, "strain%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# rc2 %le t_mark %le\n", rc2, t_mark);
  fprintf(fp, "# i ux uy drot exx eyy exy omega vol dev d2min used lost flags\n");
  for (int i = 0; i < n; ++i) {
    double exx = 0., eyy = 0., exy = 0., omega = 0., vol = 0., dev = 0.;
    if (flags[i] == 0) {
      exx = Fxx[i] - 1.; eyy = Fyy[i] - 1.;
      exy = 0.5 * (Fxy[i] + Fyx[i]); omega = 0.5 * (Fyx[i] - Fxy[i]);
      vol = exx + eyy;
      const double hh = 0.5 * (exx - eyy);
      dev = sqrt(hh * hh + exy * exy);
    }
    fprintf(fp, "%d %le %le %le %le %le %le %le %le %le %le %d %d %d\n", i, ux[i], uy[i], drot[i], exx, eyy, exy, omega, vol, dev,
            d2min[i], used[i], lost[i], flags[i]);
  }
  RC_TRY(F.close());
  // serial sums by index
  double sum_u2 = 0., sum_d2 = 0., max_d2 = 0.;
  long moved = 0, fitted = 0;
  for (int i = 0; i < n; ++i) {
    if (!(flags[i] & LBMDEM_STRAIN_NONFINITE)) { sum_u2 += ux[i] * ux[i] + uy[i] * uy[i]; ++moved; }
    if (flags[i] == 0) {
      sum_d2 += d2min[i] / (double)used[i];
      ++fitted;
      if (d2min[i] > max_d2) max_d2 = d2min[i];
    }
  }
  const double msd = moved > 0 ? sum_u2 / (double)moved : 0.;
  const double mean_d2 = fitted > 0 ? sum_d2 / (double)fitted : 0.;
  RC_TRY(F.open("a", dir, "strain.data"));
  fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0)
    fprintf(fp, "# t fitted few degenerate nonfinite_grains entries used lost worst_grain msd mean_d2min max_d2min\n");
  fprintf(fp, "%le", t);
  for (int k = 0; k < 8; ++k) fprintf(fp, " %ld", counts8[k]);
  fprintf(fp, " %le %le %le\n", msd, mean_d2, max_d2);
  return F.close();
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_strain_mark(lbmdem_handle* h, long*) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_strain_clear(lbmdem_handle* h) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_strain_compute(lbmdem_handle* h, long*) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_download_strain_grains(lbmdem_handle* h, double*, double*, double*, double*, double*, double*, double*, double*, int*, int*, int*) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_strain_grains_device(lbmdem_handle* h, const double**, const double**, const double**, const double**, const double**, const double**, const double**, const double**, const int**, const int**, const int**) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_download_strain_reference(lbmdem_handle* h, double*, double*, double*, int*, int*, long, long*, double*, long*) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_write_strain(lbmdem_handle* h, const char*, int, double, int) { SP_REFUSE(h, "the strain analysis"); }
int lbmdem_set_strain_output(lbmdem_handle* h, int, double, int) { SP_REFUSE(h, "the strain analysis"); }
#else

int lbmdem_strain_mark(lbmdem_handle* h, long* entries) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_strain_mark"));
  const auto& S = h->st;
  auto& T = h->sn;
  if (!S.valid || S.seq != h->substep_seq || S.moved != h->grains_moved)
    return fail(LBMDEM_EINVAL, "lbmdem_strain_mark: no lbmdem_structure_compute has been made for the grains where they are now");
  if (!S.listed)
    return fail(LBMDEM_EINVAL, "lbmdem_strain_mark: the last lbmdem_structure_compute had max_entries == 0: counts and "
                               "histogram only, and the mark needs its neighbour list");
  const hipStream_t st = h->stream;
  const size_t n = (size_t)h->n;
  const long total = S.entries;
  if (!T.words) {   // what depends on n, once
    HIP_TRY(h->mem.grow(&T.ref, &T.ref_cap, (long)(3 * n)));
    HIP_TRY(h->mem.grow(&T.off, &T.off_cap, (long)(n + 1)));
    HIP_TRY(h->mem.grow(&T.rec, &T.rec_cap, (long)(4 * n)));
    HIP_TRY(h->mem.grow(&T.dbl, &T.dbl_cap, (long)(8 * n)));
    HIP_TRY(h->mem.grow(&T.ints, &T.ints_cap, (long)(3 * n)));
    long words_cap = 0;
    HIP_TRY(h->mem.grow(&T.words, &words_cap, (long)SN_WORDS));   // (last: the mark of a finished allocation)
  }
  T.marked = false; T.valid = false;   // (from here on the old mark is being overwritten)
  if (total > T.nbr_cap) HIP_TRY(h->mem.grow(&T.nbr, &T.nbr_cap, total + total / 4 + 64));
  const Kin& K = h->kin[h->kcur];
  HIP_TRY(hipMemcpyAsync(T.ref, K.x1, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(T.ref + n, K.x2, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(T.ref + 2 * n, K.x3, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(T.off, S.ints + 2 * n + 1, sizeof(int) * (n + 1), hipMemcpyDeviceToDevice, st));
  if (total > 0) HIP_TRY(hipMemcpyAsync(T.nbr, S.nbr, sizeof(int) * (size_t)total, hipMemcpyDeviceToDevice, st));
  double rc2 = 0.;
  HIP_TRY(hipMemcpyAsync(&rc2, S.e2 + S.nbins, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  T.entries = total; T.rc2 = rc2; T.nbsteps = h->nbsteps;
  T.mark_gen++;
  T.marked = true;
  if (entries) *entries = total;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_strain_clear(lbmdem_handle* h) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_strain_clear"));
  h->sn.marked = false;
  h->sn.valid = false;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_strain_compute(lbmdem_handle* h, long* counts8) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts8) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_strain_compute"));
  auto& T = h->sn;
  T.valid = false;
  RC_TRY(strain_marked(h, "lbmdem_strain_compute"));
  const hipStream_t st = h->stream;
  const int n = h->n;
  const size_t N = (size_t)n;
  const Kin& K = h->kin[h->kcur];
  SnJob J{};
  J.X0 = T.ref; J.Y0 = T.ref + N; J.T0 = T.ref + 2 * N;
  J.x = K.x1; J.y = K.x2; J.th = K.x3;
  J.off = T.off; J.nbr = T.nbr;
  J.entries = T.entries;
  J.n = n;
  J.rc2 = T.rc2;
  J.rec = reinterpret_cast<double4*>(T.rec);
  J.ux = T.dbl; J.uy = T.dbl + N; J.drot = T.dbl + 2 * N; J.Fxx = T.dbl + 3 * N; J.Fxy = T.dbl + 4 * N; J.Fyx = T.dbl + 5 * N;
  J.Fyy = T.dbl + 6 * N; J.d2min = T.dbl + 7 * N;
  J.used = T.ints; J.lost = T.ints + N; J.flags = T.ints + 2 * N;
  J.words = T.words;
  HIP_TRY(hipMemsetAsync(T.words, 0, sizeof(unsigned long long) * SN_ARG, st));
  HIP_TRY(hipMemsetAsync(T.words + SN_ARG, 0xff, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_sn_pack, dim3(sn_blocks(n, SN_THREADS)), dim3(SN_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sn_fit, dim3(sn_blocks(n, SN_LANES)), dim3(SN_LANES), 0, st, J);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_sn_arg, dim3(sn_blocks(n, SN_THREADS)), dim3(SN_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[SN_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, T.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int k = 0; k < 7; ++k) counts8[k] = (long)w[k];
  counts8[7] = w[SN_FITTED] > 0 && w[SN_ARG] < (unsigned long long)n ? (long)w[SN_ARG] : -1;
  T.seq = h->substep_seq; T.moved = h->grains_moved; T.of_mark = T.mark_gen;
  T.valid = true;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_strain_grains(lbmdem_handle* h, double* ux, double* uy, double* drot, double* Fxx, double* Fxy, double* Fyx,
                                  double* Fyy, double* d2min, int* used, int* lost, int* flags) try {
  CHECK_H(h);
  RC_TRY(strain_ready(h, "lbmdem_download_strain_grains"));
  const size_t n = (size_t)h->n;
  const auto& T = h->sn;
  double* const d[8] = {ux, uy, drot, Fxx, Fxy, Fyx, Fyy, d2min};
  int* const g[3] = {used, lost, flags};
  for (int k = 0; k < 8; ++k)
    if (d[k]) HIP_TRY(hipMemcpyAsync(d[k], T.dbl + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  for (int k = 0; k < 3; ++k)
    if (g[k]) HIP_TRY(hipMemcpyAsync(g[k], T.ints + k * n, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_strain_grains_device(lbmdem_handle* h, const double** ux, const double** uy, const double** drot, const double** Fxx,
                                const double** Fxy, const double** Fyx, const double** Fyy, const double** d2min, const int** used,
                                const int** lost, const int** flags) try {
  CHECK_H(h);
  RC_TRY(strain_ready(h, "lbmdem_strain_grains_device"));
  const size_t n = (size_t)h->n;
  const auto& T = h->sn;
  const double** const d[8] = {ux, uy, drot, Fxx, Fxy, Fyx, Fyy, d2min};
  const int** const g[3] = {used, lost, flags};
  for (int k = 0; k < 8; ++k)
    if (d[k]) *d[k] = T.dbl + k * n;
  for (int k = 0; k < 3; ++k)
    if (g[k]) *g[k] = T.ints + k * n;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_strain_reference(lbmdem_handle* h, double* x0, double* y0, double* th0, int* offsets, int* nbr, long cap,
                                     long* count, double* rc2, long* nbsteps) try {
  CHECK_H(h);
  if (!count || (cap > 0 && !nbr) || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(strain_marked(h, "lbmdem_download_strain_reference"));
  const auto& T = h->sn;
  const long total = T.entries;
  *count = total;
  if (rc2) *rc2 = T.rc2;
  if (nbsteps) *nbsteps = T.nbsteps;
  if (cap > 0 && cap < total)
    return fail(LBMDEM_EINVAL, "lbmdem_download_strain_reference: there are %ld entries, the buffer holds %ld", total, cap);
  const size_t n = (size_t)h->n;
  double* const d[3] = {x0, y0, th0};
  for (int k = 0; k < 3; ++k)
    if (d[k]) HIP_TRY(hipMemcpyAsync(d[k], T.ref + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  if (offsets) HIP_TRY(hipMemcpyAsync(offsets, T.off, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, h->stream));
  if (cap > 0 && total > 0) HIP_TRY(hipMemcpyAsync(nbr, T.nbr, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_strain(lbmdem_handle* h, const char* dir, int nfile, double rcut, int incremental) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_write_strain"));
  if (!(rcut > 0) || !sn_finite(rcut)) return fail(LBMDEM_EINVAL, "lbmdem_write_strain: rcut must be finite and > 0 (%le)", rcut);
  const size_t n = (size_t)h->n;
  long scounts[8], counts[8];
  if (!h->sn.marked) {
    RC_TRY(lbmdem_structure_compute(h, rcut, 1, 1.0, (long)INT_MAX, scounts));
    RC_TRY(lbmdem_strain_mark(h, nullptr));
  }
  RC_TRY(lbmdem_strain_compute(h, counts));
  std::vector<double> d(8 * n);
  std::vector<int> g(3 * n);
  RC_TRY(lbmdem_download_strain_grains(h, d.data(), d.data() + n, d.data() + 2 * n, d.data() + 3 * n, d.data() + 4 * n,
                                       d.data() + 5 * n, d.data() + 6 * n, d.data() + 7 * n, g.data(), g.data() + n, g.data() + 2 * n));
  const double dt = h->cfg.dt;
  RC_TRY(lbmdem_write_strain_files(dir, nfile, (int)n, d.data(), d.data() + n, d.data() + 2 * n, d.data() + 3 * n, d.data() + 4 * n,
                                   d.data() + 5 * n, d.data() + 6 * n, d.data() + 7 * n, g.data(), g.data() + n, g.data() + 2 * n,
                                   h->sn.rc2, counts, h->nbsteps * dt, h->sn.nbsteps * dt));
  if (incremental) {
    RC_TRY(lbmdem_structure_compute(h, rcut, 1, 1.0, (long)INT_MAX, scounts));
    RC_TRY(lbmdem_strain_mark(h, nullptr));
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_strain_output(lbmdem_handle* h, int on, double rcut, int incremental) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_strain_output"));
    if (!(rcut > 0) || !sn_finite(rcut)) return fail(LBMDEM_EINVAL, "lbmdem_set_strain_output: rcut must be finite and > 0 (%le)", rcut);
    h->strain_rcut = rcut;
    h->strain_incremental = incremental != 0;
  }
  h->strain_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
