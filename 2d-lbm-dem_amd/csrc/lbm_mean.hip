// lbm_mean.hip -- time-averaged flow statistics (lbmdem_mean_begin, lbmdem_mean_sample, lbmdem_mean_reset, lbmdem_mean_end,
// lbmdem_mean_stats, lbmdem_mean_download, lbmdem_mean_fields, lbmdem_mean_fields_device, lbmdem_mean_profile, lbmdem_write_mean,
// lbmdem_write_mean_files, lbmdem_set_mean_output; include/lbmdem_hip.h): per-node sums over the fluid steps of a window -- the
// composite velocity and its products, the density, dissipation and shear rate of the flow-fields block, the grains' velocity,
// and how often a node was fluid or a grain's -- accumulated on the device. The reference has no such routine: the contract is the
// arithmetic the header spells out, every expression associated as written there.
//
//   k_mean_sample   a workgroup owns a window of 256 columns (lanes along y, the contiguous axis of f, obst and the planes) and a
//                   segment of MN_SEG lattice rows. One pass, no stencil: the owner is read first; a fluid node reads its nine
//                   populations (node_vel, node_moments, node_stress of lbm_device.h: the flow fields' formulas), a grain's node
//                   the five kinematics, anything else nothing. Then the node's count and the selected planes of its class are
//                   read, added to and written back, S = S + v. The mask is a uniform branch (an SGPR compare per group of planes).
//   k_mean_zero     opens or resets a window: +0.0 and 0 everywhere.
//   k_mean_fields   the derived planes [lx][ly] for the download and the torch view.
//   k_mean_profile  one lane per y marching along x: the chains of the thirteen derived values and of n_fluid.
// The planes lie at the map's row pitch (sy, a multiple of 16): a wave's row is 512 contiguous, 128-byte aligned bytes per plane.
// No atomics, no LDS: every node is read and written by exactly one lane, nothing depends on launch order. Both writing kernels are
// gated: queued behind a launch of k_dem_chain that gave up they do nothing, and the replay makes the samples again.
// With no window open nothing is allocated or launched. Double-precision library only: the entry points that take a handle refuse
// in the float build; the host-only file writer exists in both.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h), MemPool (lbm_mem.h) for the
// buffers kept on the handle, OutFile (lbm_outfile.h) for the files.
#include "lbm_device.h"
#include "lbm_outfile.h"

namespace {

constexpr int MN_FIELDS = 13;    // bits of the field mask: phi solid mux muy rxx rxy ryy mrho vrho mdiss mgdot gux guy

inline unsigned be_float(double v) {
  const float f = (float)v;
  unsigned u;
  memcpy(&u, &f, 4);
  return __builtin_bswap32(u);
}

// mean%.6i.vtk and mean_profile%.6i.dat from planes [lx][ly] and the profile [14][ly]
int mean_write_files(const char* dir, int nfile, int lx, int ly, long samples, const double* phi, const double* mux, const double* muy,
                     const double* rxx, const double* rxy, const double* ryy, const double* mrho, const double* prof) {
  const size_t cnt = (size_t)lx * ly;
  std::vector<unsigned> image(7 * cnt);   // the vector's three words per node, then four scalars
  for (int y = 0; y < ly; ++y)
    for (int x = 0; x < lx; ++x) {
      const size_t in = (size_t)x * ly + y, o = (size_t)y * lx + x;
      image[3 * o] = be_float(mux[in]);
      image[3 * o + 1] = be_float(muy[in]);
      image[3 * o + 2] = be_float(0.);
      image[3 * cnt + o] = be_float(phi[in]);
      image[4 * cnt + o] = be_float(0.5 * (rxx[in] + ryy[in]));
      image[5 * cnt + o] = be_float(rxy[in]);
      image[6 * cnt + o] = be_float(mrho[in]);
    }
  static const char* const NAMES[4] = {"fluid_fraction", "fluctuation_energy", "reynolds_xy", "mean_density"};
  {
    OutFile F;
    RC_TRY(F.open("w+", dir, "mean%.6i.vtk", nfile));
    FILE* fp = F.fp;
    lbmdem_vtk_put_mesh(fp, lx, ly);
    fprintf(fp, "VECTORS mean_fluid_velocity_lb float\n");
    bool short_write = fwrite(image.data(), 4, 3 * cnt, fp) != 3 * cnt;
    for (int k = 0; k < 4 && !short_write; ++k) {
      fprintf(fp, "SCALARS %s float\nLOOKUP_TABLE default\n", NAMES[k]);
      short_write = fwrite(image.data() + (3 + k) * cnt, 4, cnt, fp) != cnt;
    }
    RC_TRY(F.close(short_write));
  }
  OutFile F;
  RC_TRY(F.open("w+", dir, "mean_profile%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# y samples phi solid mux muy rxx rxy ryy mrho vrho mdiss mgdot gux guy\n");
  for (int y = 0; y < ly; ++y) {
    fprintf(fp, "%d %ld", y, samples);
    for (int k = 0; k < MN_FIELDS; ++k) {
      const double p = prof[(size_t)k * ly + y];
      fprintf(fp, " %le", p / (double)lx);
    }
    fprintf(fp, "\n");
  }
  return F.close(false);
}

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int MN_PLANES = 11;    // Sux Suy | Sxx Sxy Syy | Srho Srho2 | Sdiss Sgdot | Sgux Sguy
constexpr int MN_ROWS = MN_FIELDS + 1;   // the profile's rows: the thirteen fields, then n_fluid
// the first plane of each bit of the window's mask, in table order (their counts: MEAN_BIT_PLANES, lbmdem_handle.h)
constexpr int MN_BIT_FIRST[5] = {0, 2, 5, 7, 9};
// the accumulators each derived field needs
constexpr int MN_NEEDS[MN_FIELDS] = {0, 0, LBMDEM_MEAN_U, LBMDEM_MEAN_U, LBMDEM_MEAN_U | LBMDEM_MEAN_UU, LBMDEM_MEAN_U | LBMDEM_MEAN_UU,
                                     LBMDEM_MEAN_U | LBMDEM_MEAN_UU, LBMDEM_MEAN_RHO, LBMDEM_MEAN_RHO, LBMDEM_MEAN_DISS,
                                     LBMDEM_MEAN_DISS, LBMDEM_MEAN_GRAIN, LBMDEM_MEAN_GRAIN};
const char* const MN_FIELD_NAMES[MN_FIELDS] = {"phi", "solid", "mux", "muy", "rxx", "rxy", "ryy", "mrho", "vrho", "mdiss", "mgdot",
                                               "gux", "guy"};

int mn_popcount(int mask) { return __builtin_popcount((unsigned)mask); }

constexpr int MN_THREADS = 256;   // columns of a window
constexpr int MN_SEG = 16;        // rows of a segment

struct MeanJob {
  const real* f;
  const int* obst;       // device layout [x][sy]
  LatticeView L;         // (the whole lattice: gx0 == 0, nxl == lx)
  Kin K;
  double nu8, nu9;
  unsigned *nf, *ng;     // [lx][sy] each
  double* S;             // the selected planes
  long off[MN_PLANES];   // where each plane starts in S; -1: not in the window
  int mask;
};

// what the readers need of a window
struct MeanView {
  const unsigned *nf, *ng;
  const double* S;
  long off[MN_PLANES];
  int lx, ly, sy;
  double N;              // (double)samples
};

__global__ __launch_bounds__(MN_THREADS) void k_mean_sample(const MeanJob J) {
  LBMDEM_GATE(J.L.gate);
  const LatticeView& L = J.L;
  const int y = blockIdx.x * MN_THREADS + threadIdx.x;
  if (y >= L.ly) return;   // (no wave shifts, no barriers: a lane beyond the lattice has nothing to do)
  const int xa = blockIdx.y * MN_SEG;
  const int xb = xa + MN_SEG < L.lx ? xa + MN_SEG : L.lx;
  double* __restrict__ S = J.S;
  // A plane outside the node's class is left alone. The header promises S = S + v with v = +0.0 there; skipping the
  // read-modify-write gives the same bits, because a chain that starts from +0.0 never holds -0.0 (x + (+0.0) == x for every
  // other x, NaN payloads included).
#define MN_ADD(k, v) do { const long a_ = J.off[k] + at; S[a_] = S[a_] + (v); } while (0)
  for (int x = xa; x < xb; ++x) {
    const long at = (long)x * L.sy + y;
    const int o = J.obst[at];
    if (o == -1) {
      real f[9];
      const NodeVel N = node_vel(J.f, o, L, J.K, x, y, f);   // (lbm_device.h: shared with the flow fields, tracers, scalar)
      J.nf[at] = J.nf[at] + 1u;
      if (J.mask & LBMDEM_MEAN_U) { MN_ADD(0, N.ux); MN_ADD(1, N.uy); }
      if (J.mask & LBMDEM_MEAN_UU) { MN_ADD(2, N.ux * N.ux); MN_ADD(3, N.ux * N.uy); MN_ADD(4, N.uy * N.uy); }
      if (J.mask & LBMDEM_MEAN_RHO) { MN_ADD(5, N.rho); MN_ADD(6, N.rho * N.rho); }
      if (J.mask & LBMDEM_MEAN_DISS) {
        const NodeMoments P = node_moments(f);
        const NodeStress T = node_stress(L, J.nu8, J.nu9, P.pxx, P.pxy, N.rho, N.jx, N.jy);
        MN_ADD(7, T.diss); MN_ADD(8, T.gdot);
      }
    } else if (o >= 0 && o < L.n) {
      real f[9];   // (not read: a grain's node costs five kinematics loads)
      const NodeVel N = node_vel(J.f, o, L, J.K, x, y, f);
      J.ng[at] = J.ng[at] + 1u;
      if (J.mask & LBMDEM_MEAN_GRAIN) { MN_ADD(9, N.ux); MN_ADD(10, N.uy); }
    }
  }
#undef MN_ADD
}

// +0.0 into `nd` doubles, 0 into `nu` counts
__global__ __launch_bounds__(256) void k_mean_zero(const int* gate, double* __restrict__ S, long nd, unsigned* __restrict__ cnt, long nu) {
  LBMDEM_GATE(gate);
  const long stride = (long)gridDim.x * 256;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nd; k += stride) S[k] = 0.;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nu; k += stride) cnt[k] = 0u;
}

// the thirteen derived values of node `at` (the header's table); +0.0 where the divisor count is 0 and for a field whose
// accumulators the window does not hold
__device__ __forceinline__ void mn_derive(const MeanView& W, long at, double (&v)[MN_FIELDS], double& nf) {
  nf = (double)W.nf[at];
  const double ng = (double)W.ng[at];
  const bool hf = W.nf[at] != 0u, hg = W.ng[at] != 0u;
  auto plane = [&](int k, bool has) -> double { return (has && W.off[k] >= 0) ? W.S[W.off[k] + at] / (k < 9 ? nf : ng) : 0.; };
#pragma unroll
  for (int k = 0; k < MN_FIELDS; ++k) v[k] = 0.;
  v[0] = nf / W.N;
  v[1] = ng / W.N;
  const double mux = plane(0, hf), muy = plane(1, hf);
  v[2] = mux;
  v[3] = muy;
  if (hf && W.off[0] >= 0 && W.off[2] >= 0) {
    v[4] = plane(2, hf) - mux * mux;
    v[5] = plane(3, hf) - mux * muy;
    v[6] = plane(4, hf) - muy * muy;
  }
  const double mrho = plane(5, hf);
  v[7] = mrho;
  if (hf && W.off[5] >= 0) v[8] = plane(6, hf) - mrho * mrho;
  v[9] = plane(7, hf);
  v[10] = plane(8, hf);
  v[11] = plane(9, hg);
  v[12] = plane(10, hg);
}

struct MeanFieldsJob {
  MeanView W;
  double* out;              // planes [lx][ly]
  long off[MN_FIELDS];      // where each field's plane starts in out; -1: not selected
};

__global__ __launch_bounds__(MN_THREADS) void k_mean_fields(const MeanFieldsJob J) {
  const MeanView& W = J.W;
  const int y = blockIdx.x * MN_THREADS + threadIdx.x, x = blockIdx.y;
  if (y >= W.ly) return;
  double v[MN_FIELDS], nf;
  mn_derive(W, (long)x * W.sy + y, v, nf);
  const long o = (long)x * W.ly + y;
#pragma unroll
  for (int k = 0; k < MN_FIELDS; ++k)
    if (J.off[k] >= 0) J.out[J.off[k] + o] = v[k];
}

// out[14][ly]: per y the chain from +0.0 over x ascending of each derived value, and of nf
__global__ __launch_bounds__(MN_THREADS) void k_mean_profile(const MeanView W, double* __restrict__ out) {
  const int y = blockIdx.x * MN_THREADS + threadIdx.x;
  if (y >= W.ly) return;
  double a[MN_ROWS];
#pragma unroll
  for (int k = 0; k < MN_ROWS; ++k) a[k] = 0.;
  for (int x = 0; x < W.lx; ++x) {
    double v[MN_FIELDS], nf;
    mn_derive(W, (long)x * W.sy + y, v, nf);
#pragma unroll
    for (int k = 0; k < MN_FIELDS; ++k) a[k] = a[k] + v[k];
    a[MN_FIELDS] = a[MN_FIELDS] + nf;
  }
#pragma unroll
  for (int k = 0; k < MN_ROWS; ++k) out[(long)k * W.ly + y] = a[k];
}

long mn_plane(const lbmdem_handle* h) { return (long)h->L.lx * h->L.sy; }
long mn_bytes(const lbmdem_handle* h) {
  return h->mean.on ? mn_plane(h) * (long)(2 * sizeof(unsigned) + (size_t)h->mean.nsel * sizeof(double)) : 0;
}
void mn_offsets(const lbmdem_handle* h, long (&off)[MN_PLANES]) {
  int at = 0;
  for (int k = 0; k < MN_PLANES; ++k) off[k] = -1;
  for (int b = 0; b < 5; ++b)
    if ((h->mean.mask >> b) & 1)
      for (int k = 0; k < MEAN_BIT_PLANES[b]; ++k) off[MN_BIT_FIRST[b] + k] = (long)(at++) * mn_plane(h);
}
MeanView mn_view(const lbmdem_handle* h) {
  const MeanState& M = h->mean;
  MeanView W{};
  W.nf = M.cnt;
  W.ng = M.cnt + mn_plane(h);
  W.S = M.S;
  mn_offsets(h, W.off);
  W.lx = h->L.lx; W.ly = h->L.ly; W.sy = h->L.sy;
  W.N = (double)M.samples;
  return W;
}

// the window gone and its memory given back now, not when the handle ends
void mean_free(lbmdem_handle* h) {
  MeanState& M = h->mean;
  h->mem.release(M.cnt);
  h->mem.release(M.S);
  h->mem.release(M.out);
  M = MeanState{};
}

int mean_zero_launch(lbmdem_handle* h) {
  const MeanState& M = h->mean;
  const long nd = (long)M.nsel * mn_plane(h), nu = 2 * mn_plane(h);
  hipLaunchKernelGGL(k_mean_zero, dim3(grid_for(nd > nu ? nd : nu)), dim3(256), 0, h->stream, h->L.gate, M.S, nd, M.cnt, nu);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}

int mean_sample_launch(lbmdem_handle* h, const int* obst) {
  MeanState& M = h->mean;
  const LatticeView& L = h->L;
  MeanJob J{};
  J.f = h->f[h->fcur];
  J.obst = obst;
  J.L = L;
  J.K = h->kin[h->kcur];
  const double s8 = h->cfg.phys.s8, s9 = h->cfg.phys.s9;
  J.nu8 = (1. / s8 - 0.5) / 3.;   // (lbm_flow.hip's)
  J.nu9 = (1. / s9 - 0.5) / 3.;
  J.nf = M.cnt;
  J.ng = M.cnt + mn_plane(h);
  J.S = M.S;
  mn_offsets(h, J.off);
  J.mask = M.mask;
  hipLaunchKernelGGL(k_mean_sample, dim3((L.ly + MN_THREADS - 1) / MN_THREADS, (L.lx + MN_SEG - 1) / MN_SEG), dim3(MN_THREADS), 0,
                     h->stream, J);
  HIP_TRY(hipGetLastError());
  M.samples++;
  return LBMDEM_OK;
}

#define MEAN_OPEN(h, who) do { if (!(h)->mean.on) return fail(LBMDEM_EINVAL, who ": no window is open (lbmdem_mean_begin first)"); } while (0)

// what every reader of derived values checks: a window, a sample, the accumulators of every field asked for
int mean_readable(const lbmdem_handle* h, const char* who, int fmask) {
  const MeanState& M = h->mean;
  if (!M.on) return fail(LBMDEM_EINVAL, "%s: no window is open (lbmdem_mean_begin first)", who);
  if (M.samples == 0) return fail(LBMDEM_EINVAL, "%s: no sample has been taken", who);
  for (int k = 0; k < MN_FIELDS; ++k)
    if (((fmask >> k) & 1) && (MN_NEEDS[k] & ~M.mask))
      return fail(LBMDEM_EINVAL, "%s: the field %s needs accumulators that are not in the window's mask %d (it needs %d)", who,
                  MN_FIELD_NAMES[k], M.mask, MN_NEEDS[k]);
  return LBMDEM_OK;
}

// the planes of `fmask` to dev_out (device memory), on the handle's stream
int mean_fields_launch(lbmdem_handle* h, int fmask, double* dev_out) {
  const LatticeView& L = h->L;
  MeanFieldsJob J{};
  J.W = mn_view(h);
  J.out = dev_out;
  int nsel = 0;
  for (int k = 0; k < MN_FIELDS; ++k) J.off[k] = ((fmask >> k) & 1) ? (long)(nsel++) * L.lx * L.ly : -1;
  hipLaunchKernelGGL(k_mean_fields, dim3((L.ly + MN_THREADS - 1) / MN_THREADS, L.lx), dim3(MN_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}

// the fields of `fmask` that the window can give, host planes [lx][ly] each in `out` (13 planes, those not given +0.0), and the profile
int mean_host_planes(lbmdem_handle* h, int fmask, std::vector<double>& out, std::vector<double>& prof) {
  MeanState& M = h->mean;
  const LatticeView& L = h->L;
  const size_t cnt = (size_t)L.lx * L.ly;
  int can = 0;
  for (int k = 0; k < MN_FIELDS; ++k)
    if (((fmask >> k) & 1) && !(MN_NEEDS[k] & ~M.mask)) can |= 1 << k;
  const long need = (long)mn_popcount(can) * (long)cnt, total = need + (long)MN_ROWS * L.ly;
  HIP_TRY(h->mem.grow(&M.out, &M.out_cap, total));
  RC_TRY(mean_fields_launch(h, can, M.out));
  hipLaunchKernelGGL(k_mean_profile, dim3((L.ly + MN_THREADS - 1) / MN_THREADS), dim3(MN_THREADS), 0, h->stream, mn_view(h),
                     M.out + need);
  HIP_TRY(hipGetLastError());
  std::vector<double> got((size_t)total);
  HIP_TRY(hipMemcpyAsync(got.data(), M.out, sizeof(double) * got.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  out.assign(MN_FIELDS * cnt, 0.);
  size_t at = 0;
  for (int k = 0; k < MN_FIELDS; ++k)
    if ((can >> k) & 1) { memcpy(out.data() + k * cnt, got.data() + at, sizeof(double) * cnt); at += cnt; }
  prof.assign(got.begin() + need, got.end());
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

int lbmdem_mean_hook(lbmdem_handle* h, const int* obst) {
#ifdef LBMDEM_SINGLE_PRECISION
  (void)h; (void)obst;
  return fail(LBMDEM_EINVAL, "time averaging is not available in the single-precision build of the library");
#else
  MeanState& M = h->mean;
  M.hook++;
  if (M.hook % M.every != 0) return LBMDEM_OK;
  return mean_sample_launch(h, obst);
#endif
}

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_mean_files(const char* dir, int nfile, int lx, int ly, long samples, const double* phi, const double* mux,
                            const double* muy, const double* rxx, const double* rxy, const double* ryy, const double* mrho,
                            const double* profile14) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (!phi || !mux || !muy || !rxx || !rxy || !ryy || !mrho || !profile14) return fail(LBMDEM_EINVAL, "null buffer");
  if (lx < 2 || ly < 2) return fail(LBMDEM_EINVAL, "lbmdem_write_mean_files: the lattice is %d x %d", lx, ly);
  if (samples < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_mean_files: %ld samples", samples);
  return mean_write_files(dir, nfile, lx, ly, samples, phi, mux, muy, rxx, rxy, ryy, mrho, profile14);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_mean_begin(lbmdem_handle* h, int, int) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_sample(lbmdem_handle* h) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_reset(lbmdem_handle* h) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_end(lbmdem_handle* h) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_stats(lbmdem_handle* h, long*) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_download(lbmdem_handle* h, double*, unsigned*, unsigned*, long, long*) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_fields(lbmdem_handle* h, int, double*, long, long*) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_fields_device(lbmdem_handle* h, int, void*, long) { SP_REFUSE(h, "time averaging"); }
int lbmdem_mean_profile(lbmdem_handle* h, double*, long) { SP_REFUSE(h, "time averaging"); }
int lbmdem_write_mean(lbmdem_handle* h, const char*, int) { SP_REFUSE(h, "time averaging"); }
int lbmdem_set_mean_output(lbmdem_handle* h, int, int) { SP_REFUSE(h, "time averaging"); }
#else

int lbmdem_mean_begin(lbmdem_handle* h, int mask, int every) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_begin"));
  if (mask <= 0 || (mask & ~LBMDEM_MEAN_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_mean_begin: bad mask %d", mask);
  if (every < 0) return fail(LBMDEM_EINVAL, "lbmdem_mean_begin: every = %d is negative", every);
  MeanState& M = h->mean;
  if (M.on && M.mask != mask) {
    HIP_TRY(hipStreamSynchronize(h->stream));   // (a sample of the earlier window may be in flight)
    mean_free(h);
  }
  if (!M.on) {
    const long plane = mn_plane(h);
    const int nsel = mean_planes_of(mask);
    MeanState N{};
    if (h->mem.dev(&N.cnt, (size_t)(2 * plane)) != hipSuccess || h->mem.dev(&N.S, (size_t)(nsel * plane)) != hipSuccess) {
      h->mem.release(N.cnt); h->mem.release(N.S);
      return fail(LBMDEM_ENOMEM, "lbmdem_mean_begin: device allocation of %zu bytes failed",
                  (size_t)plane * (2 * sizeof(unsigned) + (size_t)nsel * sizeof(double)));
    }
    N.on = true;
    N.mask = mask;
    N.nsel = nsel;
    M = N;   // (from here on mean_free gives everything back)
  }
  M.every = every;
  M.samples = 0;
  M.hook = 0;
  M.resumed = false;   // (a window begun by hand is no loaded one; lbmdem_checkpoint_load sets the mark behind this call)
  return mean_zero_launch(h);
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_sample(lbmdem_handle* h) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_sample"));
  MEAN_OPEN(h, "lbmdem_mean_sample");
  return mean_sample_launch(h, reader_obst(h));
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_reset(lbmdem_handle* h) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_reset"));
  MEAN_OPEN(h, "lbmdem_mean_reset");
  MeanState& M = h->mean;
  M.samples = 0;
  M.hook = M.every > 0 ? M.hook % M.every : 0;
  return mean_zero_launch(h);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_end(lbmdem_handle* h) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_end"));
  if (!h->mean.on) return LBMDEM_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));   // (a sample may be in flight)
  mean_free(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_stats(lbmdem_handle* h, long* out5) try {
  CHECK_H(h);   // (settles: the counts are those of the samples that took place)
  RC_TRY(whole_handle(h, "lbmdem_mean_stats"));
  if (!out5) return fail(LBMDEM_EINVAL, "null argument");
  const MeanState& M = h->mean;
  out5[0] = M.on ? 1 : 0; out5[1] = M.mask; out5[2] = M.samples; out5[3] = M.hook; out5[4] = mn_bytes(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_download(lbmdem_handle* h, double* planes, unsigned* n_fluid, unsigned* n_grain, long cap_doubles, long* count) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_download"));
  if (!count || !n_fluid || !n_grain || cap_doubles < 0 || (cap_doubles > 0 && !planes)) return fail(LBMDEM_EINVAL, "null buffer");
  MEAN_OPEN(h, "lbmdem_mean_download");
  const MeanState& M = h->mean;
  const LatticeView& L = h->L;
  const size_t plane = (size_t)mn_plane(h), cnt = (size_t)L.lx * L.ly;
  const long need = (long)M.nsel * (long)cnt;
  *count = need;
  if (cap_doubles < need)
    return fail(LBMDEM_EINVAL, "lbmdem_mean_download: the planes are %ld doubles, the buffer holds %ld", need, cap_doubles);
  std::vector<double> sd((size_t)M.nsel * plane);
  std::vector<unsigned> cd(2 * plane);
  HIP_TRY(hipMemcpyAsync(sd.data(), M.S, sizeof(double) * sd.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(cd.data(), M.cnt, sizeof(unsigned) * cd.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int x = 0; x < L.lx; ++x)
    for (int y = 0; y < L.ly; ++y) {
      const size_t at = (size_t)x * L.sy + y, o = (size_t)x * L.ly + y;
      for (int k = 0; k < M.nsel; ++k) planes[k * cnt + o] = sd[k * plane + at];
      n_fluid[o] = cd[at];
      n_grain[o] = cd[plane + at];
    }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_fields_device(lbmdem_handle* h, int fmask, void* dev_out, long cap_doubles) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_fields_device"));
  if (fmask <= 0 || (fmask & ~LBMDEM_MEANF_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_mean_fields_device: bad mask %d", fmask);
  if (!dev_out) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(mean_readable(h, "lbmdem_mean_fields_device", fmask));
  const long need = (long)mn_popcount(fmask) * h->L.lx * h->L.ly;
  if (cap_doubles < need)
    return fail(LBMDEM_EINVAL, "lbmdem_mean_fields_device: the planes are %ld doubles, the buffer holds %ld", need, cap_doubles);
  return mean_fields_launch(h, fmask, static_cast<double*>(dev_out));
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_fields(lbmdem_handle* h, int fmask, double* out, long cap_doubles, long* count) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_fields"));
  if (fmask <= 0 || (fmask & ~LBMDEM_MEANF_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_mean_fields: bad mask %d", fmask);
  if (!count || cap_doubles < 0 || (cap_doubles > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  const long need = (long)mn_popcount(fmask) * h->L.lx * h->L.ly;
  *count = need;
  if (cap_doubles == 0) return LBMDEM_OK;   // (how many there are)
  RC_TRY(mean_readable(h, "lbmdem_mean_fields", fmask));
  if (cap_doubles < need)
    return fail(LBMDEM_EINVAL, "lbmdem_mean_fields: the planes are %ld doubles, the buffer holds %ld", need, cap_doubles);
  MeanState& M = h->mean;
  HIP_TRY(h->mem.grow(&M.out, &M.out_cap, need));
  RC_TRY(mean_fields_launch(h, fmask, M.out));
  HIP_TRY(hipMemcpyAsync(out, M.out, sizeof(double) * (size_t)need, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_mean_profile(lbmdem_handle* h, double* out, long cap_doubles) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_mean_profile"));
  if (!out) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(mean_readable(h, "lbmdem_mean_profile", 0));
  const long need = (long)MN_ROWS * h->L.ly;
  if (cap_doubles < need)
    return fail(LBMDEM_EINVAL, "lbmdem_mean_profile: the profile is %ld doubles, the buffer holds %ld", need, cap_doubles);
  MeanState& M = h->mean;
  HIP_TRY(h->mem.grow(&M.out, &M.out_cap, need));
  hipLaunchKernelGGL(k_mean_profile, dim3((h->L.ly + MN_THREADS - 1) / MN_THREADS), dim3(MN_THREADS), 0, h->stream, mn_view(h), M.out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, M.out, sizeof(double) * (size_t)need, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_mean(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_write_mean"));
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(mean_readable(h, "lbmdem_write_mean", 0));
  const int want = LBMDEM_MEANF_PHI | LBMDEM_MEANF_UX | LBMDEM_MEANF_UY | LBMDEM_MEANF_RXX | LBMDEM_MEANF_RXY | LBMDEM_MEANF_RYY |
                   LBMDEM_MEANF_RHO;
  std::vector<double> P, prof;   // (a field the window cannot give stays +0.0, as its row of the profile does)
  RC_TRY(mean_host_planes(h, want, P, prof));
  const size_t cnt = (size_t)h->L.lx * h->L.ly;
  const double* p = P.data();
  return mean_write_files(dir, nfile, h->L.lx, h->L.ly, h->mean.samples, p, p + 2 * cnt, p + 3 * cnt, p + 4 * cnt, p + 5 * cnt,
                          p + 6 * cnt, p + 7 * cnt, prof.data());
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_mean_output(lbmdem_handle* h, int mask, int every) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (mask) {
    RC_TRY(whole_handle(h, "lbmdem_set_mean_output"));
    if (mask < 0 || (mask & ~LBMDEM_MEAN_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_set_mean_output: bad mask %d", mask);
    if (every < 1) return fail(LBMDEM_EINVAL, "lbmdem_set_mean_output: every = %d, the scene samples every k-th fluid step, k >= 1", every);
  }
  h->mean_output_mask = mask;
  h->mean_output_every = mask ? every : 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
