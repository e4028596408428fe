// lbm_structure.hip -- the packing beyond touching partners: the fixed-radius neighbour list in index order, the pair histogram
// behind g(r), the bonds of the first shell, and the unnormalised bond-order and fabric sums (lbmdem_structure_compute,
// lbmdem_download_structure_grains, lbmdem_structure_grains_device, lbmdem_download_structure_hist,
// lbmdem_download_structure_neighbours, lbmdem_write_structure, lbmdem_set_structure_output, lbmdem_write_structure_files,
// lbmdem_structure_edges; include/lbmdem_hip.h has the contract in full). Integers wherever possible -- atomics may land in any
// order --, and where floating point, a chain of IEEE double operations in a stated order that one lane walks serially: no
// floating-point atomics anywhere. Nothing here is on the step path: the kernels only read the handle's state, and nothing is
// allocated or launched before the first compute.
//
// On the handle's stream:
//   k_st_bounds, k_st_grid   minimum and maximum of the finite centres as integer keys that order doubles as their bit patterns do
//                            (one atomic per wavefront), the non-finite centres counted; one lane makes the cell grid of them: the
//                            side per axis is max(rcut, extent / 1024) and a hair more (2^-20 of it, so that the rounding of a
//                            cell index cannot put two grains at exactly rcut two cells apart), at most 1025 cells per axis. The
//                            Verlet grid is not touched;
//   k_st_keys, a radix sort, k_st_gather
//                            a grain's cell (row-major; every non-finite centre in the one cell behind the last), the grains
//                            ordered by cell, their x, y, r in that order;
//   k_st_pairs<false>        the count: a workgroup of 64 lanes has 64 consecutive grains of that order. They lie in one row of
//                            cells or in several; in the first case the candidates are three runs of the order (the rows below, of,
//                            and above, each cut to the columns around the block's), in the second one run (all rows from the one
//                            below the first to the one above the last). The runs' ends are binary searches in the sorted keys; no
//                            table of cells exists, and a cell may hold any number of grains. A run is staged in LDS 256
//                            candidates at a time and every lane tests every one of them -- d2 alone decides. Per lane the
//                            neighbours and bonds; per pair i < j the histogram bin in LDS (32-bit, flushed with 64-bit atomics) and
//                            the bonded and coincident pairs; the census;
//   a scan, k_st_pairs<true> offsets[n + 1] over the counts by index, then the same walk writes the neighbours;
//   a segmented radix sort   each grain's neighbours ascending;
//   k_st_psi                 one lane per grain walks its own segment: bonds and the four sums, serially.
// No workgroup waits for another; every loop has a bound.
// Double-precision library only: the entry points that take a handle refuse in the float build; the two host-only functions
// exist in both.
// Front end, as every export's: whole_handle() and SP_REFUSE() (lbmdem_handle.h) for the refusals, MemPool::grow (lbm_mem.h) for
// the scratch kept on the handle, OutFile (lbm_outfile.h) for the files.
#include "lbm_outfile.h"

#include <errno.h>
#include <float.h>
#include <limits.h>
#include <math.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

constexpr int ST_MAX_BINS = 4096;
constexpr double ST_PI = 3.141592653589793;

bool st_finite(double v) { return v - v == 0.; }

int st_check_params(const char* who, double rcut, int nbins, double shell) {
  if (!(rcut > 0) || !st_finite(rcut)) return fail(LBMDEM_EINVAL, "%s: rcut must be finite and > 0 (%le)", who, rcut);
  if (nbins < 1 || nbins > ST_MAX_BINS) return fail(LBMDEM_EINVAL, "%s: nbins must lie in 1 .. %d (%d)", who, ST_MAX_BINS, nbins);
  if (!(shell >= 1) || !st_finite(shell)) return fail(LBMDEM_EINVAL, "%s: shell must be finite and >= 1 (%le)", who, shell);
  return LBMDEM_OK;
}

void st_edges(double rcut, int nbins, double* e2) {
  const double dr = rcut / nbins;
  for (int k = 0; k < nbins; ++k) e2[k] = ((double)k * dr) * ((double)k * dr);
  e2[nbins] = rcut * rcut;
}

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int ST_THREADS = 256;   // the per-grain kernels
constexpr int ST_WAVE = 64;       // grains of a workgroup of the pair pass
constexpr int ST_CHUNK = 256;     // candidates staged at a time
constexpr int ST_CELLS = 1024;    // extent / ST_CELLS bounds the cell side from below
constexpr int ST_KEY_BITS = 21;   // 1025 * 1025 + 1 < 2^21
// StructureStage::words: the four keys of the bounds, then the census
enum : int { ST_XMIN = 0, ST_XMAX, ST_YMIN, ST_YMAX, ST_ENTRIES, ST_BONDED, ST_MAXNB, ST_LONE, ST_SIX, ST_COINCIDENT, ST_NONFINITE,
             ST_WORDS };

struct StGrid { double x0, y0, sx, sy; int ncx, ncy; };

struct StJob {
  const double *x, *y, *r;   // the centres lbmdem_download_grain_table shows, the radii
  int n, nbins;
  double rcut, rc2, dr, shell;
  unsigned long long* words;
  StGrid* grid;
  unsigned *key, *skey;      // by index, by cell
  int *idx, *sidx;
  double *sx, *sy, *sr;      // by cell
  int *nb, *bonds, *off;     // by index; nb and off [n + 1]
  double *c6, *s6, *c2, *s2;
  const double* e2;
  unsigned long long* hist;
  int* nbr;                  // as emitted (k_st_pairs<true>) or ascending (k_st_psi)
};

// a double as an integer with the same order (lbm_clusters.hip's key)
__device__ __forceinline__ unsigned long long st_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double st_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
__device__ __forceinline__ bool st_dfinite(double v) { return v - v == 0.; }

__global__ __launch_bounds__(ST_THREADS) void k_st_bounds(const StJob J) {
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  unsigned long long xlo = ~0ull, xhi = 0ull, ylo = ~0ull, yhi = 0ull;
  bool bad = false;
  if (i < J.n) {
    const double x = J.x[i], y = J.y[i];
    if (st_dfinite(x) && st_dfinite(y)) {
      xlo = xhi = st_key(x);
      ylo = yhi = st_key(y);
    } else {
      bad = true;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {   // (every lane of the wavefront is here)
    const unsigned long long a = __shfl_xor(xlo, m), b = __shfl_xor(xhi, m), c = __shfl_xor(ylo, m), d = __shfl_xor(yhi, m);
    xlo = a < xlo ? a : xlo; xhi = b > xhi ? b : xhi;
    ylo = c < ylo ? c : ylo; yhi = d > yhi ? d : yhi;
  }
  const unsigned long long nbad = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (xlo <= xhi) {
      atomicMin(&J.words[ST_XMIN], xlo); atomicMax(&J.words[ST_XMAX], xhi);
      atomicMin(&J.words[ST_YMIN], ylo); atomicMax(&J.words[ST_YMAX], yhi);
    }
    if (nbad) atomicAdd(&J.words[ST_NONFINITE], (unsigned long long)__popcll(nbad));
  }
}

__device__ __forceinline__ void st_axis(double lo, double hi, double rcut, double* side, int* count) {
  double ext = hi - lo;
  if (!(ext <= DBL_MAX)) ext = DBL_MAX;
  double s = ext / ST_CELLS;
  if (!(s > rcut)) s = rcut;
  s = s + s * (1. / 1048576.);
  double c = ext / s;
  if (!(c < (double)ST_CELLS)) c = (double)ST_CELLS;
  *side = s;
  *count = (int)c + 1;
}

__global__ void k_st_grid(const StJob J) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  StGrid G;
  if (J.words[ST_XMIN] > J.words[ST_XMAX]) {   // no finite centre
    G.x0 = G.y0 = 0.; G.sx = G.sy = J.rcut; G.ncx = G.ncy = 1;
  } else {
    G.x0 = st_unkey(J.words[ST_XMIN]); G.y0 = st_unkey(J.words[ST_YMIN]);
    st_axis(G.x0, st_unkey(J.words[ST_XMAX]), J.rcut, &G.sx, &G.ncx);
    st_axis(G.y0, st_unkey(J.words[ST_YMAX]), J.rcut, &G.sy, &G.ncy);
  }
  *J.grid = G;
}

// monotone in v, inside [0, count)
__device__ __forceinline__ int st_cell(double v, double v0, double side, int count) {
  const double c = (v - v0) / side;
  if (!(c > 0.)) return 0;
  return c >= (double)(count - 1) ? count - 1 : (int)c;
}

__global__ __launch_bounds__(ST_THREADS) void k_st_keys(const StJob J) {
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= J.n) return;
  const StGrid G = *J.grid;
  const double x = J.x[i], y = J.y[i];
  unsigned key = (unsigned)(G.ncx * G.ncy);   // the one cell of the non-finite centres
  if (st_dfinite(x) && st_dfinite(y)) key = (unsigned)(st_cell(y, G.y0, G.sy, G.ncy) * G.ncx + st_cell(x, G.x0, G.sx, G.ncx));
  J.key[i] = key;
  J.idx[i] = i;
}

__global__ __launch_bounds__(ST_THREADS) void k_st_gather(const StJob J) {
  const int s = blockIdx.x * ST_THREADS + threadIdx.x;
  if (s >= J.n) return;
  const int i = J.sidx[s];
  J.sx[s] = J.x[i]; J.sy[s] = J.y[i]; J.sr[s] = J.r[i];
  if (s == 0) J.nb[J.n] = 0;   // the scan's last item
}

// the first place of the order whose key is >= k (n: none)
__device__ __forceinline__ int st_lower(const unsigned* skey, int n, unsigned k) {
  int lo = 0, hi = n;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int mid = lo + (hi - lo) / 2;
    if (skey[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the bin of d2: a guess from the root, corrected against the table, which alone decides
__device__ __forceinline__ int st_bin(const StJob& J, double d2) {
  const double g = sqrt(d2) / J.dr;
  int k = g >= (double)(J.nbins - 1) ? J.nbins - 1 : (g > 0. ? (int)g : 0);
  for (int step = 0; step < ST_MAX_BINS && k > 0 && d2 < J.e2[k]; ++step) --k;
  for (int step = 0; step < ST_MAX_BINS && k < J.nbins - 1 && d2 >= J.e2[k + 1]; ++step) ++k;
  return k;
}

template <bool EMIT>
__global__ __launch_bounds__(ST_WAVE) void k_st_pairs(const StJob J) {
  __shared__ double cx[ST_CHUNK], cy[ST_CHUNK], cr[ST_CHUNK];
  __shared__ int cid[ST_CHUNK];
  __shared__ int run[6];
  __shared__ unsigned lh[EMIT ? 1 : ST_MAX_BINS];
  __shared__ unsigned long long acc[6];   // entries, bonded pairs, coincident pairs, lone grains, six bonds, the most neighbours
  const int lane = threadIdx.x, n = J.n;
  const int s0 = blockIdx.x * ST_WAVE, s = s0 + lane;
  const int s1 = s0 + ST_WAVE < n ? s0 + ST_WAVE : n;   // (s0 < n by the launch)
  const StGrid G = *J.grid;
  const unsigned ncells = (unsigned)(G.ncx * G.ncy);
  if (!EMIT) {
    for (int k = lane; k < J.nbins; k += ST_WAVE) lh[k] = 0u;
    if (lane < 6) acc[lane] = 0ull;
  }
  if (lane < 6) {
    // the block's finite grains are its places [s0, f1): the non-finite ones close the order
    const int f = st_lower(J.skey, n, ncells);
    const int f1 = f < s1 ? f : s1;
    int lo = 0, hi = 0;
    if (f1 > s0) {
      const int kf = (int)J.skey[s0], kl = (int)J.skey[f1 - 1];
      const int r0 = kf / G.ncx, r1 = kl / G.ncx;
      const int d = lane >> 1;
      if (r0 == r1) {
        const int row = r0 - 1 + d;
        if (row >= 0 && row < G.ncy) {
          const int c0 = kf % G.ncx > 0 ? kf % G.ncx - 1 : 0, c1 = kl % G.ncx + 1 < G.ncx ? kl % G.ncx + 1 : G.ncx - 1;
          lo = st_lower(J.skey, n, (unsigned)(row * G.ncx + c0));
          hi = st_lower(J.skey, n, (unsigned)(row * G.ncx + c1 + 1));
        }
      } else if (d == 0) {
        const int ra = r0 > 0 ? r0 - 1 : 0, rb = r1 + 1 < G.ncy ? r1 + 1 : G.ncy - 1;
        lo = st_lower(J.skey, n, (unsigned)(ra * G.ncx));
        hi = st_lower(J.skey, n, (unsigned)((rb + 1) * G.ncx));
      }
    }
    run[lane] = (lane & 1) ? hi : lo;
  }
  __syncthreads();
  const bool mine = s < s1 && J.skey[s] < ncells;
  double xi = 0., yi = 0., ri = 0.;
  int i = -1, room = 0;
  int* out = nullptr;
  if (s < s1) i = J.sidx[s];
  if (mine) { xi = J.sx[s]; yi = J.sy[s]; ri = J.sr[s]; }
  if (EMIT && mine) {
    out = J.nbr + J.off[i];
    room = J.off[i + 1] - J.off[i];
  }
  int nb = 0, bonds = 0;
  unsigned long long bonded = 0, coincident = 0;
  long since = 0;
  for (int d = 0; d < 3; ++d) {
    const int lo = run[2 * d], hi = run[2 * d + 1];
    for (int base = lo; base < hi; base += ST_CHUNK) {
      const int cnt = hi - base < ST_CHUNK ? hi - base : ST_CHUNK;
      for (int t = lane; t < cnt; t += ST_WAVE) {
        cx[t] = J.sx[base + t]; cy[t] = J.sy[base + t]; cr[t] = J.sr[base + t]; cid[t] = J.sidx[base + t];
      }
      __syncthreads();
      if (mine) {
        for (int t = 0; t < cnt; ++t) {
          if (base + t == s) continue;
          const double dx = cx[t] - xi, dy = cy[t] - yi;
          const double d2 = dx * dx + dy * dy;
          if (!(d2 <= J.rc2)) continue;
          if (EMIT) {
            if (nb < room) out[nb] = cid[t];
            ++nb;
          } else {
            ++nb;
            const double b = J.shell * (ri + cr[t]);
            const bool bond = d2 <= b * b;
            if (bond) ++bonds;
            if (i < cid[t]) {
              atomicAdd(&lh[st_bin(J, d2)], 1u);
              if (bond) ++bonded;
              if (d2 == 0.) ++coincident;
            }
          }
        }
      }
      __syncthreads();
      if (!EMIT) {   // before 64 lanes can have added 2^32 to a 32-bit bin
        since += cnt;
        if (since >= (1l << 25)) {
          for (int k = lane; k < J.nbins; k += ST_WAVE) {
            if (lh[k]) atomicAdd(&J.hist[k], (unsigned long long)lh[k]);
            lh[k] = 0u;
          }
          since = 0;
          __syncthreads();
        }
      }
    }
  }
  if (EMIT) return;
  if (s < s1) {
    J.nb[i] = nb; J.bonds[i] = bonds;
    if (nb) atomicAdd(&acc[0], (unsigned long long)nb);
    if (bonded) atomicAdd(&acc[1], bonded);
    if (coincident) atomicAdd(&acc[2], coincident);
    if (nb == 0) atomicAdd(&acc[3], 1ull);
    if (bonds == 6) atomicAdd(&acc[4], 1ull);
    atomicMax(&acc[5], (unsigned long long)nb);
  }
  __syncthreads();
  for (int k = lane; k < J.nbins; k += ST_WAVE)
    if (lh[k]) atomicAdd(&J.hist[k], (unsigned long long)lh[k]);
  if (lane == 0) {
    if (acc[0]) atomicAdd(&J.words[ST_ENTRIES], acc[0]);
    if (acc[1]) atomicAdd(&J.words[ST_BONDED], acc[1]);
    if (acc[2]) atomicAdd(&J.words[ST_COINCIDENT], acc[2]);
    if (acc[3]) atomicAdd(&J.words[ST_LONE], acc[3]);
    if (acc[4]) atomicAdd(&J.words[ST_SIX], acc[4]);
    atomicMax(&J.words[ST_MAXNB], acc[5]);
  }
}

// one lane per grain, its neighbours ascending: the chain the contract spells out
__global__ __launch_bounds__(ST_THREADS) void k_st_psi(const StJob J) {
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= J.n) return;
  const double xi = J.x[i], yi = J.y[i], ri = J.r[i];
  double c6 = 0., s6 = 0., c2 = 0., s2 = 0.;
  const int k0 = J.off[i], k1 = J.off[i + 1];
  for (int k = k0; k < k1; ++k) {
    const int j = J.nbr[k];
    if (j < 0 || j >= J.n) continue;   // (never: the emit wrote grains)
    const double dx = J.x[j] - xi, dy = J.y[j] - yi;
    const double d2 = dx * dx + dy * dy;
    const double b = J.shell * (ri + J.r[j]);
    if (!(d2 <= b * b) || !(d2 > 0.)) continue;
    const double d = sqrt(d2), nx = dx / d, ny = dy / d;
    const double a2 = nx * nx - ny * ny, b2 = 2. * nx * ny;
    const double a4 = a2 * a2 - b2 * b2, b4 = 2. * a2 * b2;
    const double a6 = a4 * a2 - b4 * b2, b6 = b4 * a2 + a4 * b2;
    c2 += a2; s2 += b2; c6 += a6; s6 += b6;
  }
  J.c6[i] = c6; J.s6[i] = s6; J.c2[i] = c2; J.s2[i] = s2;
}

int st_blocks(long items, int threads) { return (int)((items + threads - 1) / threads); }

int st_bits(int n) {   // the bits of a grain index
  int b = 1;
  while (b < 31 && (1l << b) < (long)n) ++b;
  return b;
}

// what depends on n, once; hipcub's scratch for the sort by cell and the scan
int structure_stage(lbmdem_handle* h) {
  auto& S = h->st;
  const size_t n = (size_t)h->n;
  if (S.words) return LBMDEM_OK;
  StGrid* grid = nullptr;
  HIP_TRY(h->mem.dev(&grid, 1));
  S.grid = grid;
  HIP_TRY(h->mem.dev(&S.keys, 2 * n));
  HIP_TRY(h->mem.dev(&S.idx, 2 * n));
  HIP_TRY(h->mem.dev(&S.sorted, 3 * n));
  HIP_TRY(h->mem.dev(&S.ints, 3 * n + 2));
  HIP_TRY(h->mem.dev(&S.sums, 4 * n));
  HIP_TRY(h->mem.dev(&S.e2, (size_t)ST_MAX_BINS + 1));
  HIP_TRY(h->mem.dev(&S.hist, (size_t)ST_MAX_BINS));
  size_t a = 0, b = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, a, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr, (int*)nullptr, (int)n,
                                             0, ST_KEY_BITS, h->stream));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int*)nullptr, (int*)nullptr, (int)n + 1, h->stream));
  HIP_TRY(h->mem.grow(&S.tmp, &S.tmp_bytes, (long)(a > b ? a : b)));
  HIP_TRY(h->mem.dev(&S.words, (size_t)ST_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

int structure_ready(const lbmdem_handle* h, const char* who, bool list) {
  RC_TRY(whole_handle(h, who));
  const auto& S = h->st;
  if (!S.valid || S.seq != h->substep_seq || S.moved != h->grains_moved)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_structure_compute has been made for the grains where they are now", who);
  if (list && !S.listed)
    return fail(LBMDEM_EINVAL, "%s: the last lbmdem_structure_compute had max_entries == 0: counts and histogram only", who);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_structure_edges(double rcut, int nbins, double* e2) {
  if (!e2) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(st_check_params("lbmdem_structure_edges", rcut, nbins, 1.));
  st_edges(rcut, nbins, e2);
  return LBMDEM_OK;
}

int lbmdem_write_structure_files(const char* dir, int nfile, int n, const int* nb, const int* bonds, const double* c6, const double* s6,
                                 const double* c2, const double* s2, double rcut, int nbins, double shell, const long* hist,
                                 const long* counts8, double t, double W, double H) try {
  if (n < 1 || !nb || !bonds || !c6 || !s6 || !c2 || !s2 || !hist || !counts8)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_structure_files arguments");
  RC_TRY(st_check_params("lbmdem_write_structure_files", rcut, nbins, shell));
  for (int i = 0; i < n; ++i)
    if (nb[i] < 0 || nb[i] >= n || bonds[i] < 0 || bonds[i] > nb[i])
      return fail(LBMDEM_EINVAL, "lbmdem_write_structure_files: grain %d has %d neighbours and %d bonds among %d grains", i, nb[i],
                  bonds[i], n);
  for (int k = 0; k < nbins; ++k)
    if (hist[k] < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_structure_files: bin %d holds %ld pairs", k, hist[k]);
  std::vector<double> e2((size_t)nbins + 1);
  st_edges(rcut, nbins, e2.data());
  OutFile F;
  RC_TRY(F.open("w", dir, "structure%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# rcut %le nbins %d shell %le\n", rcut, nbins, shell);
  fprintf(fp, "# i neighbours bonds c6 s6 c2 s2\n");
  for (int i = 0; i < n; ++i) fprintf(fp, "%d %d %d %le %le %le %le\n", i, nb[i], bonds[i], c6[i], s6[i], c2[i], s2[i]);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "gr%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# rcut %le nbins %d n %d W %le H %le\n", rcut, nbins, n, W, H);
  fprintf(fp, "# k r_lo r_hi count g; g = count / (((n (n - 1) / 2 * pi) * (e2[k+1] - e2[k])) / (W * H)), 0 where that is no "
              "positive number; no edge correction\n");
  const double npairs_all = ((double)n * (double)(n - 1)) / 2.;
  for (int k = 0; k < nbins; ++k) {
    const double ideal = ((npairs_all * ST_PI) * (e2[k + 1] - e2[k])) / (W * H);
    const double g = ideal > 0 ? (double)hist[k] / ideal : 0.;
    fprintf(fp, "%d %le %le %ld %le\n", k, sqrt(e2[k]), sqrt(e2[k + 1]), hist[k], g);
  }
  RC_TRY(F.close());
  // the two order parameters: serial sums by index
  double psi = 0., C2 = 0., S2 = 0.;
  long with = 0, B = 0;
  for (int i = 0; i < n; ++i) {
    C2 += c2[i]; S2 += s2[i];
    B += bonds[i];
    if (bonds[i] > 0) { psi += sqrt(c6[i] * c6[i] + s6[i] * s6[i]) / (double)bonds[i]; ++with; }
  }
  const double psi6 = with > 0 ? psi / (double)with : 0.;
  const double fabric = B > 0 ? sqrt(C2 * C2 + S2 * S2) / (double)B : 0.;
  RC_TRY(F.open("a", dir, "structure.data"));
  fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0)
    fprintf(fp, "# t entries pairs bonded_pairs max_neighbours lone_grains six_bonds coincident_pairs nonfinite_grains psi6 fabric\n");
  fprintf(fp, "%le", t);
  for (int k = 0; k < 8; ++k) fprintf(fp, " %ld", counts8[k]);
  fprintf(fp, " %le %le\n", psi6, fabric);
  return F.close();
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_structure_compute(lbmdem_handle* h, double, int, double, long, long*) { SP_REFUSE(h, "the packing structure analysis"); }
int lbmdem_download_structure_grains(lbmdem_handle* h, int*, int*, double*, double*, double*, double*) { SP_REFUSE(h, "the packing structure analysis"); }
int lbmdem_structure_grains_device(lbmdem_handle* h, const int**, const int**, const double**, const double**, const double**, const double**) { SP_REFUSE(h, "the packing structure analysis"); }
int lbmdem_download_structure_hist(lbmdem_handle* h, long*, int, int*) { SP_REFUSE(h, "the packing structure analysis"); }
int lbmdem_download_structure_neighbours(lbmdem_handle* h, int*, int*, long, long*) { SP_REFUSE(h, "the packing structure analysis"); }
int lbmdem_write_structure(lbmdem_handle* h, const char*, int, double, int, double) { SP_REFUSE(h, "the packing structure analysis"); }
int lbmdem_set_structure_output(lbmdem_handle* h, int, double, int, double) { SP_REFUSE(h, "the packing structure analysis"); }
#else

int lbmdem_structure_compute(lbmdem_handle* h, double rcut, int nbins, double shell, long max_entries, long* counts8) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts8) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_structure_compute"));
  RC_TRY(st_check_params("lbmdem_structure_compute", rcut, nbins, shell));
  if (max_entries < 0 || max_entries > (long)INT_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_structure_compute: max_entries must lie in 0 .. %d (%ld)", INT_MAX, max_entries);
  auto& S = h->st;
  S.valid = false;
  RC_TRY(structure_stage(h));
  const int n = h->n;
  StJob J{};
  J.x = h->kin[h->kcur].x1; J.y = h->kin[h->kcur].x2; J.r = h->r;
  J.n = n; J.nbins = nbins;
  J.rcut = rcut; J.rc2 = rcut * rcut; J.dr = rcut / nbins; J.shell = shell;
  J.words = S.words;
  J.grid = static_cast<StGrid*>(S.grid);
  J.key = S.keys; J.skey = S.keys + n;
  J.idx = S.idx; J.sidx = S.idx + n;
  J.sx = S.sorted; J.sy = S.sorted + n; J.sr = S.sorted + 2 * (size_t)n;
  J.nb = S.ints; J.bonds = S.ints + n + 1; J.off = S.ints + 2 * (size_t)n + 1;
  J.c6 = S.sums; J.s6 = S.sums + n; J.c2 = S.sums + 2 * (size_t)n; J.s2 = S.sums + 3 * (size_t)n;
  J.e2 = S.e2; J.hist = S.hist;
  const hipStream_t st = h->stream;
  std::vector<double> e2((size_t)nbins + 1);
  st_edges(rcut, nbins, e2.data());
  unsigned long long w[ST_WORDS] = {};
  w[ST_XMIN] = w[ST_YMIN] = ~0ull;
  HIP_TRY(hipMemcpyAsync(S.words, w, sizeof w, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(S.e2, e2.data(), sizeof(double) * e2.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(S.hist, 0, sizeof(unsigned long long) * ST_MAX_BINS, st));
  const int gb = st_blocks(n, ST_THREADS), wb = st_blocks(n, ST_WAVE);
  hipLaunchKernelGGL(k_st_bounds, dim3(gb), dim3(ST_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_st_grid, dim3(1), dim3(64), 0, st, J);
  hipLaunchKernelGGL(k_st_keys, dim3(gb), dim3(ST_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  size_t bytes = (size_t)S.tmp_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(S.tmp, bytes, J.key, J.skey, J.idx, J.sidx, n, 0, ST_KEY_BITS, st));
  hipLaunchKernelGGL(k_st_gather, dim3(gb), dim3(ST_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_st_pairs<false>, dim3(wb), dim3(ST_WAVE), 0, st, J);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(w, S.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // (e2 and w may go now)
  const unsigned long long entries = w[ST_ENTRIES];
  if (max_entries > 0 && entries > (unsigned long long)max_entries)
    return fail(LBMDEM_EINVAL, "lbmdem_structure_compute: the list has %llu entries, max_entries is %ld", entries, max_entries);
  S.listed = false;
  if (max_entries > 0) {
    if (entries > 0) {
      HIP_TRY(h->mem.grow(&S.nbr, &S.nbr_cap, (long)(2 * entries + entries / 4 + 64)));
      size_t need = 0;
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, need, (int*)nullptr, (int*)nullptr, (int)entries, n, J.off, J.off + 1,
                                                         0, st_bits(n), st));
      if ((long)need > S.tmp_bytes) HIP_TRY(h->mem.grow(&S.tmp, &S.tmp_bytes, (long)need));
    }
    bytes = (size_t)S.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(S.tmp, bytes, J.nb, J.off, n + 1, st));
    if (entries > 0) {
      int* raw = S.nbr + S.nbr_cap / 2;   // as emitted; the first half takes them ascending
      J.nbr = raw;
      hipLaunchKernelGGL(k_st_pairs<true>, dim3(wb), dim3(ST_WAVE), 0, st, J);
      HIP_TRY(hipGetLastError());
      bytes = (size_t)S.tmp_bytes;
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(S.tmp, bytes, raw, S.nbr, (int)entries, n, J.off, J.off + 1, 0, st_bits(n), st));
    }
    J.nbr = S.nbr;
    hipLaunchKernelGGL(k_st_psi, dim3(gb), dim3(ST_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    S.listed = true;
  }
  counts8[0] = (long)entries;
  counts8[1] = (long)(entries / 2);
  counts8[2] = (long)w[ST_BONDED];
  counts8[3] = (long)w[ST_MAXNB];
  counts8[4] = (long)w[ST_LONE];
  counts8[5] = (long)w[ST_SIX];
  counts8[6] = (long)w[ST_COINCIDENT];
  counts8[7] = (long)w[ST_NONFINITE];
  S.entries = (long)entries; S.nbins = nbins;
  S.seq = h->substep_seq; S.moved = h->grains_moved;
  S.valid = true;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_structure_grains(lbmdem_handle* h, int* nb, int* bonds, double* c6, double* s6, double* c2, double* s2) try {
  CHECK_H(h);
  RC_TRY(structure_ready(h, "lbmdem_download_structure_grains", true));
  const size_t n = (size_t)h->n;
  const auto& S = h->st;
  if (nb) HIP_TRY(hipMemcpyAsync(nb, S.ints, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  if (bonds) HIP_TRY(hipMemcpyAsync(bonds, S.ints + n + 1, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  double* const dst[4] = {c6, s6, c2, s2};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], S.sums + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_structure_grains_device(lbmdem_handle* h, const int** nb, const int** bonds, const double** c6, const double** s6,
                                   const double** c2, const double** s2) try {
  CHECK_H(h);
  RC_TRY(structure_ready(h, "lbmdem_structure_grains_device", true));
  const size_t n = (size_t)h->n;
  const auto& S = h->st;
  if (nb) *nb = S.ints;
  if (bonds) *bonds = S.ints + n + 1;
  if (c6) *c6 = S.sums;
  if (s6) *s6 = S.sums + n;
  if (c2) *c2 = S.sums + 2 * n;
  if (s2) *s2 = S.sums + 3 * n;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_structure_hist(lbmdem_handle* h, long* hist, int cap, int* nbins) try {
  CHECK_H(h);
  if (!nbins || (cap > 0 && !hist) || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(structure_ready(h, "lbmdem_download_structure_hist", false));
  const int total = h->st.nbins;
  *nbins = total;
  if (cap == 0) return LBMDEM_OK;   // (how many bins there are)
  if (cap < total) return fail(LBMDEM_EINVAL, "lbmdem_download_structure_hist: there are %d bins, the buffer holds %d", total, cap);
  static_assert(sizeof(long) == sizeof(unsigned long long), "the histogram's words");
  HIP_TRY(hipMemcpyAsync(hist, h->st.hist, sizeof(long) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_structure_neighbours(lbmdem_handle* h, int* offsets, int* nbr, long cap, long* count) try {
  CHECK_H(h);
  if (!count || (cap > 0 && !nbr) || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(structure_ready(h, "lbmdem_download_structure_neighbours", true));
  const auto& S = h->st;
  const long total = S.entries;
  *count = total;
  if (cap == 0 && !offsets) return LBMDEM_OK;   // (how many there are)
  if (cap > 0 && cap < total)
    return fail(LBMDEM_EINVAL, "lbmdem_download_structure_neighbours: there are %ld entries, the buffer holds %ld", total, cap);
  const size_t n = (size_t)h->n;
  if (offsets) HIP_TRY(hipMemcpyAsync(offsets, S.ints + 2 * n + 1, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, h->stream));
  if (cap > 0 && total > 0) HIP_TRY(hipMemcpyAsync(nbr, S.nbr, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_structure(lbmdem_handle* h, const char* dir, int nfile, double rcut, int nbins, double shell) try {
  CHECK_H(h);
  const int n = h->n;
  long counts[8];
  RC_TRY(lbmdem_structure_compute(h, rcut, nbins, shell, (long)INT_MAX, counts));
  std::vector<int> g(2 * (size_t)n);
  std::vector<double> d(4 * (size_t)n);
  RC_TRY(lbmdem_download_structure_grains(h, g.data(), g.data() + n, d.data(), d.data() + n, d.data() + 2 * (size_t)n,
                                          d.data() + 3 * (size_t)n));
  std::vector<long> hist((size_t)nbins);
  int got = 0;
  RC_TRY(lbmdem_download_structure_hist(h, hist.data(), nbins, &got));
  const lbmdem_config& c = h->cfg;
  return lbmdem_write_structure_files(dir, nfile, n, g.data(), g.data() + n, d.data(), d.data() + n, d.data() + 2 * (size_t)n,
                                      d.data() + 3 * (size_t)n, rcut, nbins, shell, hist.data(), counts, h->nbsteps * c.dt,
                                      c.Mdx - c.Mgx, c.Mhy - c.Mby);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_structure_output(lbmdem_handle* h, int on, double rcut, int nbins, double shell) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_structure_output"));
    RC_TRY(st_check_params("lbmdem_set_structure_output", rcut, nbins, shell));
    h->structure_rcut = rcut; h->structure_nbins = nbins; h->structure_shell = shell;
  }
  h->structure_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
