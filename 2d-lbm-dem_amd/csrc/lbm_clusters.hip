// lbm_clusters.hip -- force chains: the contact net of the last table sub-step read as a graph (lbmdem_cluster_compute,
// lbmdem_download_cluster_grains, lbmdem_cluster_grains_device, lbmdem_download_clusters, lbmdem_cluster_rounds,
// lbmdem_write_clusters, lbmdem_set_clusters_output, lbmdem_write_clusters_files; include/lbmdem_hip.h). The records of
// lbm_contacts.hip stay on the device (lbmdem_contacts_records); the records at or above a force threshold are the edges, the
// grains the nodes, the walls no nodes. Every result is an integer, or a minimum or maximum, that does not depend on the order of
// evaluation: atomics are free to land in any order, and the contract is equality with a serial restatement. The one floating-point
// sum, the mean force of a relative threshold, is a chain of additions in a fixed order. Nothing here is on the step path: the
// kernels only read the handle's state.
//
// On the handle's stream:
//   k_cl_partials, k_cl_threshold   S and m: one lane per block of 1024 pair records adds its block serially, one lane the partials;
//   k_cl_init, k_cl_select          a record's selection byte, degree[] and walls[] by atomics, the two record counters;
//   k_cl_hook, k_cl_flatten         components, in rounds: every selected pair finds the roots of its ends (the parent of a node is
//                                   never larger than the node, so a walk descends and ends after at most n steps) and hooks the
//                                   larger root under the smaller with atomicMin; then every grain points at its root. A hook that
//                                   lowered a word raises `changed`; the host stops at the first quiet round, in which every pair
//                                   found one root for both ends: each component is one tree, its root its smallest grain. Every
//                                   round but the quiet one turns at least one root into a child and nothing makes a root: at most
//                                   n rounds. Parent words are read and written through relaxed agent-scope atomics only (another
//                                   workgroup, on another XCD, may write them in the same launch);
//   k_cl_peel, k_cl_peel_pairs      the core, in rounds: round t removes every grain still there whose remaining degree is below
//                                   zmin, then every selected pair with an end removed in round t takes one off the other end's
//                                   remaining degree. The first round that removes nothing ends it: at most n + 1 rounds;
//   k_cl_grains, k_cl_records, k_cl_roots, a scan, k_cl_emit
//                                   per root the size, the walls, the core members, the box and the pair records by atomics; "is a
//                                   root of size >= 2" scanned into the table's slots, ascending label; the census.
// No workgroup waits for another; every device loop has a bound, and the walk to a root raises `error` where it hits its own.
// Double-precision library only: the entry points that take a handle refuse in the float build; the files' formatter is host code
// and exists in both.
// Front end, as every export's: whole_handle() and SP_REFUSE() (lbmdem_handle.h) for the refusals, MemPool::grow (lbm_mem.h) for
// the scratch kept on the handle, OutFile (lbm_outfile.h) for the files.
#include "lbm_outfile.h"

#include <errno.h>
#include <float.h>
#include <limits.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

static_assert(sizeof(lbmdem_cluster) == 56 && offsetof(lbmdem_cluster, contacts) == 8 && offsetof(lbmdem_cluster, walls) == 16 &&
              offsetof(lbmdem_cluster, xmin) == 24, "lbmdem_cluster's layout");

// the palette of DEM%.6i_clusters.ps, indexed by label % 8 (include/lbmdem_hip.h lists it)
const char* const CL_PALETTE[8] = {"0.894 0.102 0.110", "0.216 0.494 0.722", "0.302 0.686 0.290", "0.596 0.306 0.639",
                                   "1.000 0.498 0.000", "0.651 0.337 0.157", "0.969 0.506 0.749", "0.400 0.400 0.400"};

bool cl_selected(double fn, double thr) { return fn >= thr; }   // (false for NaN)

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int CL_THREADS = 256;
constexpr int CL_BLOCK = 1024;   // records per block partial of S
// the planes of ClusterStage::ints, [n] each, the last one [n + 1]; the scan's positions [n + 1] follow them
enum : int { CL_PARENT = 0, CL_DEGREE, CL_WALLS, CL_CORE, CL_REM, CL_GONE, CL_SIZE, CL_CWALLS, CL_CCORE, CL_FLAG, CL_INT_PLANES };
enum : int { CL_CHANGED = 10, CL_ERROR = 11, CL_WORDS = 12 };   // ClusterStage::census behind the ten counts

struct ClusterJob {
  const lbmdem_contact* rec;
  long npairs, nrec;
  int n, zmin, round;
  double fmin;
  int relative;
  const double *x1, *x2;       // the centres lbmdem_download_grain_table shows
  int *parent, *degree, *walls, *core, *rem, *gone, *size, *cwalls, *ccore, *flag, *pos;
  unsigned long long *contacts, *box;   // [n]; [4][n] keys of xmin, xmax, ymin, ymax
  unsigned long long* census;  // [CL_WORDS]
  double* thr;
  double* partial;             // [nb]
  long long* pcount;           // [nb]
  long nb;
  unsigned char* sel;
  lbmdem_cluster* table;
};

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_raise(unsigned long long* w) {
  __hip_atomic_store(w, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one atomic per wavefront: the lanes with `pred` counted (every lane of the wavefront calls)
__device__ __forceinline__ void cl_count(unsigned long long* w, bool pred) {
  const unsigned long long m = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(w, (unsigned long long)__popcll(m));
}
// a double as an integer with the same order (-0.0 below +0.0, a NaN beyond the infinity of its sign), and back
__device__ __forceinline__ unsigned long long cl_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double cl_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
__device__ __forceinline__ void cl_ends(const lbmdem_contact* rec, long k, int* i, int* j) {
  const int2 ij = *reinterpret_cast<const int2*>(rec + k);
  *i = ij.x; *j = ij.y;
}

// S, first level: lane b chains the fn > 0 of the pair records [1024 b, 1024 (b + 1)) from +0.0, ascending
__global__ __launch_bounds__(CL_THREADS) void k_cl_partials(const ClusterJob J) {
  const long b = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (b >= J.nb) return;
  const long k0 = b * CL_BLOCK, k1 = k0 + CL_BLOCK < J.npairs ? k0 + CL_BLOCK : J.npairs;
  double s = 0.;
  long long m = 0;
  for (long k = k0; k < k1; ++k) {
    const double fn = J.rec[k].fn;
    if (fn > 0) { s += fn; ++m; }
  }
  J.partial[b] = s;
  J.pcount[b] = m;
}

// S, second level, and the threshold: one lane
__global__ void k_cl_threshold(const ClusterJob J) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double thr = J.fmin;
  if (J.relative) {
    double S = 0.;
    long long m = 0;
    for (long b = 0; b < J.nb; ++b) { S += J.partial[b]; m += J.pcount[b]; }
    if (m == 0) thr = J.fmin > 0 ? __builtin_inf() : 0.;
    else thr = J.fmin * (S / (double)m);
  }
  *J.thr = thr;
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_init(const ClusterJob J) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= J.n) return;
  J.parent[i] = i;
  J.degree[i] = 0; J.walls[i] = 0; J.gone[i] = 0;
  J.size[i] = 0; J.cwalls[i] = 0; J.ccore[i] = 0;
  J.contacts[i] = 0;
  const size_t n = (size_t)J.n;
  J.box[i] = ~0ull; J.box[n + i] = 0; J.box[2 * n + i] = ~0ull; J.box[3 * n + i] = 0;
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_select(const ClusterJob J) {
  const long k = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  bool pair = false, wall = false;
  if (k < J.nrec) {
    const bool s = J.rec[k].fn >= *J.thr;   // (false for NaN)
    J.sel[k] = s ? 1 : 0;
    if (s) {
      int i, j;
      cl_ends(J.rec, k, &i, &j);
      atomicAdd(&J.degree[i], 1);
      if (j >= 0) { pair = true; atomicAdd(&J.degree[j], 1); }
      else { wall = true; atomicOr(&J.walls[i], 1 << (-j - 1)); }
    }
  }
  cl_count(&J.census[0], pair);
  cl_count(&J.census[1], wall);
}

// the root of x: parents descend, so at most n steps; more is an error, reported and not waited for
__device__ __forceinline__ int cl_root(const ClusterJob& J, int x) {
  for (int s = 0; s <= J.n; ++s) {
    const int p = cl_load(J.parent + x);
    if (p == x) return x;
    x = p;
  }
  cl_raise(&J.census[CL_ERROR]);
  return x;
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_hook(const ClusterJob J) {
  const long k = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (k >= J.npairs || !J.sel[k]) return;
  int i, j;
  cl_ends(J.rec, k, &i, &j);
  const int ri = cl_root(J, i), rj = cl_root(J, j);
  if (ri == rj) return;
  const int hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
  if (atomicMin(&J.parent[hi], lo) > lo) cl_raise(&J.census[CL_CHANGED]);
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_flatten(const ClusterJob J) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= J.n) return;
  const int p = cl_load(J.parent + i);
  if (p == i) return;
  const int root = cl_root(J, p);
  if (root != p) cl_store(J.parent + i, root);   // (an ancestor, and not above the old one)
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_peel(const ClusterJob J) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= J.n) return;
  if (J.gone[i] == 0 && J.rem[i] < J.zmin) {
    J.gone[i] = J.round;
    cl_raise(&J.census[CL_CHANGED]);
  }
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_peel_pairs(const ClusterJob J) {
  const long k = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (k >= J.npairs || !J.sel[k]) return;
  int i, j;
  cl_ends(J.rec, k, &i, &j);
  if (J.gone[i] == J.round) atomicSub(&J.rem[j], 1);
  if (J.gone[j] == J.round) atomicSub(&J.rem[i], 1);
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_grains(const ClusterJob J) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  bool lone = false, core = false;
  if (i < J.n) {
    core = J.gone[i] == 0;
    lone = J.degree[i] == 0;
    J.core[i] = core ? 1 : 0;
    const int L = J.parent[i];
    atomicAdd(&J.size[L], 1);
    const int w = J.walls[i];
    if (w) atomicOr(&J.cwalls[L], w);
    if (core) atomicAdd(&J.ccore[L], 1);
    const size_t n = (size_t)J.n;
    const unsigned long long kx = cl_key(J.x1[i]), ky = cl_key(J.x2[i]);
    atomicMin(&J.box[L], kx); atomicMax(&J.box[n + L], kx);
    atomicMin(&J.box[2 * n + L], ky); atomicMax(&J.box[3 * n + L], ky);
  }
  cl_count(&J.census[5], lone);
  cl_count(&J.census[6], core);
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_records(const ClusterJob J) {
  const long k = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  bool cpair = false, cwall = false;
  if (k < J.nrec && J.sel[k]) {
    int i, j;
    cl_ends(J.rec, k, &i, &j);
    const bool ci = J.gone[i] == 0;
    if (j >= 0) {
      atomicAdd(&J.contacts[J.parent[i]], 1ull);
      cpair = ci && J.gone[j] == 0;
    } else {
      cwall = ci;
    }
  }
  cl_count(&J.census[7], cpair);
  cl_count(&J.census[8], cwall);
}

// lanes 0 .. n: lane n writes the flag behind the last grain, whose position is the number of entries
__global__ __launch_bounds__(CL_THREADS) void k_cl_roots(const ClusterJob J) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  bool entry = false;
  if (i < J.n) {
    const int sz = J.size[i];
    if (J.parent[i] == i) {
      entry = sz >= 2;
      // the largest size, the smallest label among equals
      atomicMax(&J.census[3], ((unsigned long long)(unsigned)sz << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
      const int w = J.cwalls[i];
      const unsigned long long span = ((w & 12) == 12 ? 1ull : 0ull) | ((w & 3) == 3 ? 2ull : 0ull);
      if (span) atomicOr(&J.census[9], span);
    }
    J.flag[i] = entry ? 1 : 0;
  } else if (i == J.n) {
    J.flag[i] = 0;
  }
  cl_count(&J.census[2], entry);
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_emit(const ClusterJob J) {
  const int i = blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= J.n || !J.flag[i]) return;
  const size_t n = (size_t)J.n;
  lbmdem_cluster c;
  c.label = i; c.size = J.size[i];
  c.contacts = (long)J.contacts[i];
  c.walls = J.cwalls[i]; c.core = J.ccore[i];
  c.xmin = cl_unkey(J.box[i]); c.xmax = cl_unkey(J.box[n + i]);
  c.ymin = cl_unkey(J.box[2 * n + i]); c.ymax = cl_unkey(J.box[3 * n + i]);
  J.table[J.pos[i]] = c;   // (at most n / 2 roots have two members)
}

int cl_blocks(long items) { return (int)((items + CL_THREADS - 1) / CL_THREADS); }

// scratch of the handle's pool: what depends on n once, what depends on the record count grown with it
int cluster_stage(lbmdem_handle* h, long nrec, long nb) {
  auto& C = h->cl;
  const size_t n = (size_t)h->n;
  if (!C.ints) {
    HIP_TRY(h->mem.dev(&C.words, 5 * n));
    HIP_TRY(h->mem.dev(&C.census, (size_t)CL_WORDS));
    HIP_TRY(h->mem.dev(&C.thr, 1));
    HIP_TRY(h->mem.dev(&C.table, n / 2 + 1));
    size_t bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (int*)nullptr, (int*)nullptr, (int)n + 1, h->stream));
    HIP_TRY(h->mem.dev(&C.scan_tmp, bytes));
    C.scan_bytes = bytes;
    HIP_TRY(h->mem.dev(&C.ints, (size_t)CL_INT_PLANES * n + 1 + n + 1));
  }
  if (C.sel_cap < nrec) HIP_TRY(h->mem.grow(&C.sel, &C.sel_cap, nrec + nrec / 8 + 64));
  if (C.partial_cap < 2 * nb) HIP_TRY(h->mem.grow(&C.partial, &C.partial_cap, 2 * nb + 16));
  return LBMDEM_OK;
}

// the words of the loops, after a round
int cluster_words(lbmdem_handle* h, unsigned long long* w2) {
  HIP_TRY(hipMemcpyAsync(w2, h->cl.census + CL_CHANGED, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
}

int clusters_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  if (!h->contacts_valid || h->contacts_walls != h->walls_moved || !h->cl.valid || h->cl.seq != h->substep_seq)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_cluster_compute has been made for the last table sub-step", who);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_clusters_files(const char* dir, int nfile, int n, const double* r, const double* x1, const double* x2,
                                const double* fm, const lbmdem_contact* c, long count, const int* label, const int* degree,
                                const int* core, const int* walls, const lbmdem_cluster* table, long nclusters, double fmin,
                                int relative, int zmin, double thr, const long* counts10, double t, int lx, int ly) {
  if (n < 1 || !r || !x1 || !x2 || !fm || count < 0 || (count > 0 && !c) || !label || !degree || !core || !walls || nclusters < 0 ||
      (nclusters > 0 && !table) || !counts10)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_clusters_files arguments");
  for (long k = 0; k < count; ++k) {
    const bool wall = c[k].j <= LBMDEM_WALL_B && c[k].j >= LBMDEM_WALL_R;
    if (c[k].i < 0 || c[k].i >= n || (!wall && (c[k].j < 0 || c[k].j >= n)))
      return fail(LBMDEM_EINVAL, "lbmdem_write_clusters_files: record %ld names a grain outside [0, %d) or an unknown wall", k, n);
  }
  for (int i = 0; i < n; ++i)
    if (label[i] < 0 || label[i] >= n)
      return fail(LBMDEM_EINVAL, "lbmdem_write_clusters_files: the label of grain %d lies outside [0, %d)", i, n);
  OutFile F;
  RC_TRY(F.open("w", dir, "clusters%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# fmin %le relative %d zmin %d threshold %le\n", fmin, relative, zmin, thr);
  fprintf(fp, "# i label degree core walls\n");
  for (int i = 0; i < n; ++i) fprintf(fp, "%d %d %d %d %d\n", i, label[i], degree[i], core[i], walls[i]);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "cluster_table%.6i.dat", nfile));
  fp = F.fp;
  for (long k = 0; k < nclusters; ++k) {
    const lbmdem_cluster& e = table[k];
    fprintf(fp, "%d %d %ld %d %d %le %le %le %le\n", e.label, e.size, e.contacts, e.walls, e.core, e.xmin, e.xmax, e.ymin, e.ymax);
  }
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "DEM%.6i_clusters.ps", nfile));
  fp = F.fp;
  lbmdem_ps_head(fp, n, x1, x2, r, fm, 1, lx, ly);
  for (long k = 0; k < count; ++k) {
    if (c[k].j < 0 || !cl_selected(c[k].fn, thr)) continue;   // walls have no second centre
    const int i = c[k].i, j = c[k].j;
    fprintf(fp, "%le setlinewidth \n %s setrgbcolor \n", c[k].fn, CL_PALETTE[label[i] % 8]);
    fprintf(fp, "1 setlinecap \n newpath \n");
    fprintf(fp, "%le %le moveto \n %le %le lineto\n", x1[i] * 10000, x2[i] * 10000, x1[j] * 10000, x2[j] * 10000);
    fprintf(fp, "stroke \n");
  }
  RC_TRY(F.close());
  RC_TRY(F.open("a", dir, "clusters.data"));
  fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0)
    fprintf(fp, "# t threshold selected_pairs selected_walls clusters largest_size largest_label isolated_grains core_grains "
                "core_pairs core_walls spanning\n");
  fprintf(fp, "%le %le", t, thr);
  for (int k = 0; k < 10; ++k) fprintf(fp, " %ld", counts10[k]);
  fprintf(fp, "\n");
  return F.close();
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_cluster_compute(lbmdem_handle* h, double, int, int, long*, double*) { SP_REFUSE(h, "the cluster analysis"); }
int lbmdem_download_cluster_grains(lbmdem_handle* h, int*, int*, int*, int*) { SP_REFUSE(h, "the cluster analysis"); }
int lbmdem_cluster_grains_device(lbmdem_handle* h, const int**, const int**, const int**, const int**) { SP_REFUSE(h, "the cluster analysis"); }
int lbmdem_download_clusters(lbmdem_handle* h, lbmdem_cluster*, long, long*) { SP_REFUSE(h, "the cluster analysis"); }
int lbmdem_cluster_rounds(lbmdem_handle* h, int*) { SP_REFUSE(h, "the cluster analysis"); }
int lbmdem_write_clusters(lbmdem_handle* h, const char*, int, double, int, int) { SP_REFUSE(h, "the cluster analysis"); }
int lbmdem_set_clusters_output(lbmdem_handle* h, int, double, int, int) { SP_REFUSE(h, "the cluster analysis"); }
#else

int lbmdem_cluster_compute(lbmdem_handle* h, double fmin, int relative, int zmin, long* counts10, double* thr) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10 || !thr) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_cluster_compute"));
  if (!(fmin >= 0) || !(fmin <= DBL_MAX)) return fail(LBMDEM_EINVAL, "lbmdem_cluster_compute: fmin must be finite and >= 0 (%le)", fmin);
  if (zmin < 0 || zmin > 6) return fail(LBMDEM_EINVAL, "lbmdem_cluster_compute: zmin must lie in 0 .. 6 (%d)", zmin);
  auto& C = h->cl;
  C.valid = false;
  long npairs = 0, nrec = 0;
  RC_TRY(lbmdem_contacts_records(h, "lbmdem_cluster_compute", LONG_MAX, &npairs, &nrec));
  const int n = h->n;
  const long nb = (npairs + CL_BLOCK - 1) / CL_BLOCK;
  RC_TRY(cluster_stage(h, nrec, nb));
  ClusterJob J{};
  J.rec = h->cx.rec;
  J.npairs = npairs; J.nrec = nrec;
  J.n = n; J.zmin = zmin;
  J.fmin = fmin; J.relative = relative != 0;
  J.x1 = h->kin[h->kcur].x1; J.x2 = h->kin[h->kcur].x2;
  int* I = C.ints;
  J.parent = I + (size_t)CL_PARENT * n; J.degree = I + (size_t)CL_DEGREE * n; J.walls = I + (size_t)CL_WALLS * n;
  J.core = I + (size_t)CL_CORE * n; J.rem = I + (size_t)CL_REM * n; J.gone = I + (size_t)CL_GONE * n;
  J.size = I + (size_t)CL_SIZE * n; J.cwalls = I + (size_t)CL_CWALLS * n; J.ccore = I + (size_t)CL_CCORE * n;
  J.flag = I + (size_t)CL_FLAG * n;   // [n + 1]: the last plane is one longer, the positions [n + 1] follow it
  J.pos = I + (size_t)CL_INT_PLANES * n + 1;
  J.contacts = C.words; J.box = C.words + n;
  J.census = C.census; J.thr = C.thr;
  J.partial = C.partial; J.pcount = reinterpret_cast<long long*>(C.partial + nb);
  J.nb = nb;
  J.sel = C.sel; J.table = C.table;
  const hipStream_t st = h->stream;
  const int gb = cl_blocks(n), rb = cl_blocks(nrec), pb = cl_blocks(npairs);
  HIP_TRY(hipMemsetAsync(C.census, 0, CL_WORDS * sizeof(unsigned long long), st));
  if (J.relative && nb > 0) hipLaunchKernelGGL(k_cl_partials, dim3(cl_blocks(nb)), dim3(CL_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_cl_threshold, dim3(1), dim3(64), 0, st, J);
  hipLaunchKernelGGL(k_cl_init, dim3(gb), dim3(CL_THREADS), 0, st, J);
  if (rb > 0) hipLaunchKernelGGL(k_cl_select, dim3(rb), dim3(CL_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[2] = {0, 0};
  // components: until a round hooks nothing
  C.rounds_cc = 0;
  for (int round = 1; pb > 0; ++round) {
    if (round > n + 1) return fail(LBMDEM_EINVAL, "lbmdem_cluster_compute: the components did not settle in %d rounds", n + 1);
    HIP_TRY(hipMemsetAsync(C.census + CL_CHANGED, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_cl_hook, dim3(pb), dim3(CL_THREADS), 0, st, J);
    hipLaunchKernelGGL(k_cl_flatten, dim3(gb), dim3(CL_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    RC_TRY(cluster_words(h, w));
    if (w[1]) return fail(LBMDEM_EINVAL, "lbmdem_cluster_compute: a walk to a root did not end within %d steps", n);
    C.rounds_cc = round;
    if (!w[0]) break;
  }
  // the core: until a round removes nothing
  HIP_TRY(hipMemcpyAsync(J.rem, J.degree, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
  C.rounds_core = 0;
  for (int round = 1; zmin > 0; ++round) {
    if (round > n + 1) return fail(LBMDEM_EINVAL, "lbmdem_cluster_compute: the core did not settle in %d rounds", n + 1);
    J.round = round;
    HIP_TRY(hipMemsetAsync(C.census + CL_CHANGED, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_cl_peel, dim3(gb), dim3(CL_THREADS), 0, st, J);
    if (pb > 0) hipLaunchKernelGGL(k_cl_peel_pairs, dim3(pb), dim3(CL_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    RC_TRY(cluster_words(h, w));
    if (!w[0]) break;
    C.rounds_core = round;   // (the rounds that removed something)
  }
  hipLaunchKernelGGL(k_cl_grains, dim3(gb), dim3(CL_THREADS), 0, st, J);
  if (rb > 0) hipLaunchKernelGGL(k_cl_records, dim3(rb), dim3(CL_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_cl_roots, dim3(cl_blocks((long)n + 1)), dim3(CL_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  size_t bytes = C.scan_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(C.scan_tmp, bytes, J.flag, J.pos, n + 1, st));
  hipLaunchKernelGGL(k_cl_emit, dim3(gb), dim3(CL_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long c[10];
  double t = 0.;
  HIP_TRY(hipMemcpyAsync(c, C.census, sizeof c, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&t, C.thr, sizeof t, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int k = 0; k < 10; ++k) counts10[k] = (long)c[k];
  counts10[3] = (long)(c[3] >> 32);                                  // the key of k_cl_roots
  counts10[4] = (long)(0xFFFFFFFFu - (unsigned)(c[3] & 0xFFFFFFFFull));
  *thr = t;
  C.nclusters = (long)c[2]; C.npairs = npairs; C.nrec = nrec;
  C.seq = h->substep_seq;
  C.valid = true;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_cluster_grains(lbmdem_handle* h, int* label, int* degree, int* core, int* walls) try {
  CHECK_H(h);
  RC_TRY(clusters_ready(h, "lbmdem_download_cluster_grains"));
  const size_t n = (size_t)h->n;
  int* const dst[4] = {label, degree, core, walls};
  const int plane[4] = {CL_PARENT, CL_DEGREE, CL_CORE, CL_WALLS};
  for (int k = 0; k < 4; ++k)
    if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], h->cl.ints + plane[k] * n, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_cluster_grains_device(lbmdem_handle* h, const int** label, const int** degree, const int** core, const int** walls) try {
  CHECK_H(h);
  RC_TRY(clusters_ready(h, "lbmdem_cluster_grains_device"));
  const size_t n = (size_t)h->n;
  if (label) *label = h->cl.ints + CL_PARENT * n;
  if (degree) *degree = h->cl.ints + CL_DEGREE * n;
  if (core) *core = h->cl.ints + CL_CORE * n;
  if (walls) *walls = h->cl.ints + CL_WALLS * n;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_clusters(lbmdem_handle* h, lbmdem_cluster* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || (cap > 0 && !out) || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(clusters_ready(h, "lbmdem_download_clusters"));
  const long total = h->cl.nclusters;
  *count = total;
  if (cap == 0) return LBMDEM_OK;   // (how many there are)
  if (cap < total) return fail(LBMDEM_EINVAL, "lbmdem_download_clusters: there are %ld entries, the buffer holds %ld", total, cap);
  if (total == 0) return LBMDEM_OK;
  HIP_TRY(hipMemcpyAsync(out, h->cl.table, sizeof(lbmdem_cluster) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_cluster_rounds(lbmdem_handle* h, int* rounds2) try {
  CHECK_H(h);
  if (!rounds2) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(clusters_ready(h, "lbmdem_cluster_rounds"));
  rounds2[0] = h->cl.rounds_cc;
  rounds2[1] = h->cl.rounds_core;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_clusters(lbmdem_handle* h, const char* dir, int nfile, double fmin, int relative, int zmin) try {
  CHECK_H(h);
  const int n = h->n;
  long counts[10];
  double thr = 0.;
  RC_TRY(lbmdem_cluster_compute(h, fmin, relative, zmin, counts, &thr));
  const long count = h->cl.nrec, ncl = h->cl.nclusters;
  std::vector<lbmdem_contact> rec((size_t)(count > 0 ? count : 1));
  if (count > 0) {   // (the records the compute has left on the device)
    HIP_TRY(hipMemcpyAsync(rec.data(), h->cx.rec, sizeof(lbmdem_contact) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  std::vector<int> g(4 * (size_t)n);
  RC_TRY(lbmdem_download_cluster_grains(h, g.data(), g.data() + n, g.data() + 2 * (size_t)n, g.data() + 3 * (size_t)n));
  std::vector<lbmdem_cluster> table((size_t)(ncl > 0 ? ncl : 1));
  long got = 0;
  if (ncl > 0) RC_TRY(lbmdem_download_clusters(h, table.data(), ncl, &got));
  std::vector<double> t(30 * (size_t)n), col(4 * (size_t)n);
  RC_TRY(lbmdem_download_grain_table(h, t.data()));
  double *r = col.data(), *x1 = r + n, *x2 = x1 + n, *fm = x2 + n;
  for (int i = 0; i < n; ++i) {
    const double* o = &t[(size_t)i * 30];
    r[i] = o[9]; x1[i] = o[0]; x2[i] = o[1]; fm[i] = o[18];
  }
  return lbmdem_write_clusters_files(dir, nfile, n, r, x1, x2, fm, rec.data(), count, g.data(), g.data() + n, g.data() + 2 * (size_t)n,
                                     g.data() + 3 * (size_t)n, table.data(), ncl, fmin, relative != 0, zmin, thr, counts,
                                     h->nbsteps * h->cfg.dt, h->cfg.lx, h->cfg.ly);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_clusters_output(lbmdem_handle* h, int on, double fmin, int relative, int zmin) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_clusters_output"));
    if (!(fmin >= 0) || !(fmin <= DBL_MAX)) return fail(LBMDEM_EINVAL, "lbmdem_set_clusters_output: fmin must be finite and >= 0 (%le)", fmin);
    if (zmin < 0 || zmin > 6) return fail(LBMDEM_EINVAL, "lbmdem_set_clusters_output: zmin must lie in 0 .. 6 (%d)", zmin);
    h->clusters_fmin = fmin; h->clusters_relative = relative != 0; h->clusters_zmin = zmin;
  }
  h->clusters_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
