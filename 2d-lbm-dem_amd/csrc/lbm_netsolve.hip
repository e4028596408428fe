// lbm_netsolve.hip -- network pressures: the pore network as a resistor network. Every link gets a conductance from its width, the
// regions that touch an inlet side are held at pressure 1 and those that touch an outlet side at 0, Kirchhoff's equations are
// solved for the others by a Jacobi-preconditioned conjugate gradient, and the flow per link, the net inflow per region and the
// totals are read off (lbmdem_netsolve_compute, lbmdem_download_netsolve_regions, lbmdem_download_netsolve_links,
// lbmdem_netsolve_rounds, lbmdem_write_netsolve, lbmdem_set_netsolve_output, lbmdem_write_netsolve_files; include/lbmdem_hip.h,
// "Network pressures", has the contract in full). The arithmetic is spelled out there operation by operation: every row is a chain
// in ascending link index, every dot product one fixed tree, so a numpy restatement reproduces every double on the bits and nothing
// depends on the order anything happens in or on how the host batches the launches. Nothing here is on the step path: the kernels
// read the NetworkStage's label plane and tables of the level and write to the handle's NetsolveStage; nothing is allocated or
// launched before the first compute.
//
// On the handle's stream, one lane per region or link unless stated, workgroups of 256:
//   k_ns_ends     per link the two regions (level 1: the rank of the root body in the group table, a binary search) and g;
//   (hipcub)      a stable radix sort of (hi, link): the links below each region, in ascending link index;
//   k_ns_first    per region the first link with lo >= it and the first sorted entry with hi >= it: the row of region a is the
//                 sorted run of hi == a, then the table's own run of lo == a, and starts at the sum of the two firsts;
//   k_ns_emit     the rows as (partner, g), every entry to the place those firsts give it: no atomics;
//   k_ns_band     one lane per node: a fluid node of from's or to's REGION sets its bit in the body's (root body's) word;
//   k_ns_flags    flags and their census;
//   k_ns_rows     serial over the row: degree, diag, b; x = 0, r = b, z, and the block's part of rz0;
//   k_ns_a        launch A of iteration k: every workgroup reduces the parts of dot(r, z) that launch B of iteration k - 1 left
//                 (k == 1: k_ns_rows) and makes the stop tests of iteration k - 1 from those bits; then d = z + beta * d for its own
//                 regions into the other d buffer and on the fly for its rows' partners, q = apply(d), the block's part of dq;
//   k_ns_b        launch B: every workgroup reduces the parts of dq, makes the dq test, updates x, r, z, leaves its part of
//                 dot(r, z). Lane 0 of workgroup 0 publishes rz, the iteration count and the status; a set status is read once
//                 per workgroup, and both kernels return at once behind it. k is a kernel argument, so nothing a launch reads is
//                 written in that launch except the status, whose every reader comes to the same decision itself;
//   k_ns_out      q per link, p and net per region, the blocks' parts of Q_in and Q_out, flowing links, the largest |q|;
//   k_ns_last     the two totals, and the smallest index among the links that hold that |q|.
// No workgroup waits for another, no floating-point atomics, no grid-wide barrier; integer atomics for the bits and the counts.
// Every loop has the bound its comment states.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both. Front end, as every export's: whole_handle(), SP_REFUSE() (lbmdem_handle.h), MemPool (lbm_mem.h), OutFile (lbm_outfile.h),
// lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>
#include <math.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

constexpr int NS_SIDE_MAX = 32768;   // the clearance analysis': a node's index < 2^30

#ifndef LBMDEM_SINGLE_PRECISION
typedef unsigned long long ns_u64;
constexpr int NS_THREADS = 256;      // rule 4's block of 256 entries is a workgroup
constexpr long NS_REGIONS_MAX = 256L * 256 * 256;   // three levels of rule 4
constexpr int NS_BATCH = 16;         // iterations the host enqueues between two reads of the status
constexpr int NS_AUTO_CAP = 100000;  // max_iter == 0: the free regions, at most this
// NetsolveStage::words
enum : int { NS_W_STATUS = 0, NS_W_ITER, NS_W_INLET, NS_W_OUTLET, NS_W_SHORTED, NS_W_FREE, NS_W_FLOWING, NS_W_TOP, NS_W_TOP_LINK, NS_WORDS };
// NetsolveStage::scal
enum : int { NS_S_RZ0 = 0, NS_S_LAST, NS_S_RZK, NS_S_QIN = NS_S_RZK + 2, NS_S_QOUT, NS_SCAL };

struct NsJob {
  const int* lab;    // [lx][sy] the network's body or group plane: a body's number, -1 off the fluid and in the pad columns
  int lx, ly, sy;
  long N;            // lx * sy
  int from, to, band;
  int level, model;
  long B, R, L;      // body numbers, regions, links
  const lbmdem_net_link* links;     // [L] of the level, ascending (lo, hi)
  const lbmdem_net_body* bodies;    // [B]
  const lbmdem_net_group* groups;   // level 1: [R]
  const double* g_user;             // model 1: [L] on the device
  int *ea, *eb;      // [L] the regions of a link's ends
  double* g;         // [L]
  int *iota, *skey, *sval;   // [L] the sort: link numbers, hi sorted, the links in that order
  int *flo, *fhi;    // [R + 1]
  int* cp;           // [2L] the rows: partner
  double* cg;        // [2L] ... and g
  unsigned* bits;    // [B] by body number: 1 an inlet node, 2 an outlet node
  int* flags;        // [R]
  double *diag, *b, *x, *r, *z, *q, *d[2];   // [R]
  double *part_dq, *part_rz, *part_in, *part_out;   // [nblk]
  int nblk;          // blocks of 256 regions
  ns_u64* words;
  double* scal;
  lbmdem_netsolve_region* regions;   // [R]
  lbmdem_netsolve_link* out;         // [L]
  double tol2;
  int max_iter;
};

__device__ __forceinline__ bool ns_region(const NsJob& J, int mask, int x, int y) {   // drainage's REGION
  return ((mask & 1) && y < J.band) || ((mask & 2) && y >= J.ly - J.band) || ((mask & 4) && x < J.band) || ((mask & 8) && x >= J.lx - J.band);
}

// rule 4 over one block of 256 entries, by one wavefront: the steps of 128 and 64 as each lane's four entries, the steps of 32 .. 1
// along the lanes (after the step of s the lanes below s hold what the tree holds there). v[i] is +0.0 from n on. -> lane 0
// (every lane of the wavefront is here)
__device__ __forceinline__ double ns_tree(const double* v, int n, int lane) {
  const double a0 = lane < n ? v[lane] : 0., a1 = lane + 64 < n ? v[lane + 64] : 0.;
  const double a2 = lane + 128 < n ? v[lane + 128] : 0., a3 = lane + 192 < n ? v[lane + 192] : 0.;
  double t = (a0 + a2) + (a1 + a3);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) t = t + __shfl_down(t, s);
  return t;
}

// a workgroup's 256 addends -> its block's value in part[blockIdx.x] (every thread of the workgroup is here)
__device__ __forceinline__ void ns_block_part(double t, double* s_t, double* part) {
  s_t[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < 64) {
    const double v = ns_tree(s_t, NS_THREADS, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
  }
}

// rule 4 from its second level on: the n >= 1 block values of an earlier launch -> the one value, in every thread. n <= 65536, so
// at most 256 blocks of them (64 per wavefront) and one more level. (every thread of the workgroup is here)
__device__ __forceinline__ double ns_total(const double* part, int n, double* s_red) {
  if (n == 1) return part[0];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = (n + 255) >> 8;
  for (int c = wave; c < m && c < NS_THREADS; c += NS_THREADS / 64) {
    const double v = ns_tree(part + (long)c * 256, n - c * 256 < 256 ? n - c * 256 : 256, lane);
    if (lane == 0) s_red[c] = v;
  }
  __syncthreads();
  double out;
  if (m == 1) out = s_red[0];
  else out = __shfl(ns_tree(s_red, m < NS_THREADS ? m : NS_THREADS, lane), 0);   // (each wavefront for itself)
  __syncthreads();   // (s_red may be used again)
  return out;
}

// the status as the workgroup sees it, read once: lane 0 of workgroup 0 may set it while this launch runs
__device__ __forceinline__ bool ns_stopped(const NsJob& J, int* s_stop) {
  if (threadIdx.x == 0) *s_stop = __hip_atomic_load(J.words + NS_W_STATUS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  __syncthreads();
  return *s_stop != 0;
}

__device__ __forceinline__ void ns_publish(const NsJob& J, int status, int iterations) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    J.words[NS_W_ITER] = (ns_u64)iterations;
    __hip_atomic_store(J.words + NS_W_STATUS, (ns_u64)(status + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ int ns_rank(const NsJob& J, int body) {   // the place of a root body in the group table: 32 halvings at most
  long a = 0, e = J.R;
  while (a < e) {
    const long m = (a + e) >> 1;
    if (J.groups[m].body < body) a = m + 1; else e = m;
  }
  return a < J.R && J.groups[a].body == body ? (int)a : -1;
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_ends(const NsJob J) {
  const long t = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  if (t >= J.L) return;
  const lbmdem_net_link e = J.links[t];
  int a = e.lo, b = e.hi, na = 0, nb = 0;
  bool ok = a >= 0 && a < J.B && b >= 0 && b < J.B;   // (always)
  if (ok && J.level) { a = ns_rank(J, a); b = ns_rank(J, b); ok = a >= 0 && b >= 0 && a < b; }
  double g = 0.;
  if (ok) {
    na = J.level ? J.groups[a].node : J.bodies[a].node;
    nb = J.level ? J.groups[b].node : J.bodies[b].node;
    if (J.model == 0) {
      const int dx = nb / J.ly - na / J.ly, dy = nb % J.ly - na % J.ly;
      const double w = 2.0 * sqrt((double)e.saddle);
      const double len = sqrt((double)(dx * dx + dy * dy));
      g = ((w * w) * w) / (12.0 * len);
    } else {
      g = J.g_user[t];
    }
  }
  J.ea[t] = ok ? a : 0;   // (never 0, 0 with g = 0: a link has two regions)
  J.eb[t] = ok ? b : 0;
  J.g[t] = g;
  J.iota[t] = (int)t;
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_first(const NsJob J) {
  const long r = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  if (r > J.R) return;
  long a = 0, e = J.L;   // the first link with lo >= r, the first sorted entry with hi >= r: 32 halvings at most each
  while (a < e) {
    const long m = (a + e) >> 1;
    if ((long)J.ea[m] < r) a = m + 1; else e = m;
  }
  J.flo[r] = (int)a;
  a = 0; e = J.L;
  while (a < e) {
    const long m = (a + e) >> 1;
    if ((long)J.skey[m] < r) a = m + 1; else e = m;
  }
  J.fhi[r] = (int)a;
}

// row a: the entries j of the sorted run of hi == a at flo[a] + j, then the links t of lo == a at fhi[a + 1] + t
__global__ __launch_bounds__(NS_THREADS) void k_ns_emit(const NsJob J) {
  const long j = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  if (j >= J.L) return;
  {
    const int lo = J.ea[j];
    const long pos = (long)J.fhi[lo + 1] + j;
    if (pos >= 0 && pos < 2 * J.L) { J.cp[pos] = J.eb[j]; J.cg[pos] = J.g[j]; }   // (always inside)
  }
  {
    const int t = J.sval[j], hi = J.skey[j];
    const long pos = (long)J.flo[hi] + j;
    if (t >= 0 && t < J.L && pos >= 0 && pos < 2 * J.L) { J.cp[pos] = J.ea[t]; J.cg[pos] = J.g[t]; }
  }
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_band(const NsJob J) {
  const long node = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  if (node >= J.N) return;
  const int x = (int)(node / J.sy), y = (int)(node % J.sy);
  if (y >= J.ly) return;
  const unsigned bit = (ns_region(J, J.from, x, y) ? 1u : 0u) | (ns_region(J, J.to, x, y) ? 2u : 0u);
  if (!bit) return;
  const int l = J.lab[node];
  if (l < 0 || l >= J.B) return;   // (no fluid here)
  atomicOr(&J.bits[l], bit);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_flags(const NsJob J) {
  const long a = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  int f = -1;
  if (a < J.R) {
    const long body = J.level ? (long)J.groups[a].body : a;
    const unsigned bit = body >= 0 && body < J.B ? J.bits[body] : 0u;
    f = (bit & 1u) ? ((bit & 2u) ? 5 : 1) : (bit & 2u) ? 2 : 0;
    J.flags[a] = f;
  }
  const ns_u64 nin = __popcll(__ballot(f > 0 && (f & 1))), nout = __popcll(__ballot(f == 2));
  const ns_u64 nsh = __popcll(__ballot(f > 0 && (f & 4))), nfree = __popcll(__ballot(f == 0));
  if ((threadIdx.x & 63) == 0) {
    if (nin) atomicAdd(&J.words[NS_W_INLET], nin);
    if (nout) atomicAdd(&J.words[NS_W_OUTLET], nout);
    if (nsh) atomicAdd(&J.words[NS_W_SHORTED], nsh);
    if (nfree) atomicAdd(&J.words[NS_W_FREE], nfree);
  }
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_rows(const NsJob J) {
  __shared__ double s_t[NS_THREADS];
  const long a = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  double t = 0.;
  if (a < J.R) {
    const long j0 = (long)J.flo[a] + J.fhi[a], j1 = (long)J.flo[a + 1] + J.fhi[a + 1];
    const bool is_free = J.flags[a] == 0;
    double diag = 0., b = 0.;
    for (long j = j0; j < j1 && j < 2 * J.L; ++j) {   // the row: at most 2L entries
      const double g = J.cg[j];
      diag = diag + g;
      if (is_free && (J.flags[J.cp[j]] & 1)) b = b + g;
    }
    const double z = is_free && diag > 0. ? b / diag : 0.;
    J.diag[a] = diag; J.b[a] = b;
    J.x[a] = 0.; J.r[a] = b; J.z[a] = z;
    J.d[0][a] = 0.; J.d[1][a] = 0.; J.q[a] = 0.;
    J.regions[a].flags = J.flags[a];
    J.regions[a].degree = (int)(j1 - j0);
    t = b * z;
  }
  ns_block_part(t, s_t, J.part_rz);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_a(const NsJob J, const int k) {
  __shared__ double s_t[NS_THREADS];
  __shared__ double s_red[NS_THREADS];
  __shared__ int s_stop;
  if (ns_stopped(J, &s_stop)) return;
  const double rzn = ns_total(J.part_rz, J.nblk, s_red);   // dot(r, z) as iteration k - 1 left it; k == 1: rz0
  const bool herald = blockIdx.x == 0 && threadIdx.x == 0;
  double beta = 0.;
  if (herald) J.scal[NS_S_LAST] = rzn;
  if (k == 1) {
    if (herald) J.scal[NS_S_RZ0] = rzn;
    if (rzn == 0.) { ns_publish(J, 0, 0); return; }
  } else {
    const double rz0 = J.scal[NS_S_RZ0];   // (of launch A of iteration 1)
    if (rzn <= J.tol2 * rz0) { ns_publish(J, 0, k - 1); return; }
    if (k - 1 >= J.max_iter) { ns_publish(J, 1, k - 1); return; }
    beta = rzn / J.scal[NS_S_RZK + ((k - 1) & 1)];   // (of launch A of iteration k - 1)
  }
  if (herald) J.scal[NS_S_RZK + (k & 1)] = rzn;   // this iteration's rz: launch B reads it, the next launch A divides by it
  const double* dold = J.d[(k - 1) & 1];
  double* dnew = J.d[k & 1];
  const long a = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  double t = 0.;
  if (a < J.R) {
    const double da = k == 1 ? J.z[a] : J.z[a] + beta * dold[a];
    dnew[a] = da;
    double qa = 0.;
    if (J.flags[a] == 0) {
      const long j0 = (long)J.flo[a] + J.fhi[a], j1 = (long)J.flo[a + 1] + J.fhi[a + 1];
      double s = 0.;
      for (long j = j0; j < j1 && j < 2 * J.L; ++j) {   // the row: at most 2L entries
        const int p = J.cp[j];
        const double dp = k == 1 ? J.z[p] : J.z[p] + beta * dold[p];
        s = s + J.cg[j] * dp;
      }
      qa = J.diag[a] * da - s;
    }
    J.q[a] = qa;
    t = da * qa;
  }
  ns_block_part(t, s_t, J.part_dq);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_b(const NsJob J, const int k) {
  __shared__ double s_t[NS_THREADS];
  __shared__ double s_red[NS_THREADS];
  __shared__ int s_stop;
  if (ns_stopped(J, &s_stop)) return;
  const double dq = ns_total(J.part_dq, J.nblk, s_red);
  if (!(dq > 0.) || !(dq < INFINITY)) { ns_publish(J, 2, k - 1); return; }   // x stays as before
  const double alpha = J.scal[NS_S_RZK + (k & 1)] / dq;
  const double* d = J.d[k & 1];
  const long a = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  double t = 0.;
  if (a < J.R) {
    J.x[a] = J.x[a] + alpha * d[a];
    const double r = J.r[a] - alpha * J.q[a];
    const double diag = J.diag[a];
    const double z = J.flags[a] == 0 && diag > 0. ? r / diag : 0.;
    J.r[a] = r; J.z[a] = z;
    t = r * z;
  }
  ns_block_part(t, s_t, J.part_rz);
}

__device__ __forceinline__ double ns_p(const NsJob& J, int a) {
  const int f = J.flags[a];
  return (f & 1) ? 1.0 : (f & 2) ? 0.0 : J.x[a];
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_out(const NsJob J) {
  __shared__ double s_t[NS_THREADS];
  const long i = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  bool flowing = false;
  ns_u64 top = 0;
  if (i < J.L) {
    const double g = J.g[i];
    const double q = g * (ns_p(J, J.ea[i]) - ns_p(J, J.eb[i]));
    J.out[i].g = g; J.out[i].q = q;
    flowing = q != 0.;
    top = (ns_u64)__double_as_longlong(fabs(q));
  }
  const ns_u64 nflow = __popcll(__ballot(flowing));
  for (int m = 32; m >= 1; m >>= 1) { const ns_u64 o = __shfl_xor(top, m); top = o > top ? o : top; }
  if ((threadIdx.x & 63) == 0) {
    if (nflow) atomicAdd(&J.words[NS_W_FLOWING], nflow);
    if (top) atomicMax(&J.words[NS_W_TOP], top);
  }
  if ((int)blockIdx.x >= J.nblk) return;   // (the whole workgroup: blocks beyond the regions)
  double tin = 0., tout = 0.;
  if (i < J.R) {
    const long j0 = (long)J.flo[i] + J.fhi[i], j1 = (long)J.flo[i + 1] + J.fhi[i + 1];
    const double p = ns_p(J, (int)i);
    double net = 0.;
    for (long j = j0; j < j1 && j < 2 * J.L; ++j) net = net + J.cg[j] * (ns_p(J, J.cp[j]) - p);   // the row: at most 2L entries
    J.regions[i].p = p; J.regions[i].net = net;
    const int f = J.flags[i];
    if (f & 1) tin = -net;
    else if (f & 2) tout = net;
  }
  ns_block_part(tin, s_t, J.part_in);
  __syncthreads();
  ns_block_part(tout, s_t, J.part_out);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_last(const NsJob J) {
  __shared__ double s_red[NS_THREADS];
  const long i = (long)blockIdx.x * NS_THREADS + threadIdx.x;
  const ns_u64 top = J.words[NS_W_TOP];   // (k_ns_out has finished)
  ns_u64 mine = ~0ull;
  if (i < J.L && (ns_u64)__double_as_longlong(fabs(J.out[i].q)) == top) mine = (ns_u64)i;
  for (int m = 32; m >= 1; m >>= 1) { const ns_u64 o = __shfl_xor(mine, m); mine = o < mine ? o : mine; }
  if ((threadIdx.x & 63) == 0 && mine != ~0ull) atomicMin(&J.words[NS_W_TOP_LINK], mine);
  if (blockIdx.x == 0 && J.nblk > 0) {
    const double qin = ns_total(J.part_in, J.nblk, s_red), qout = ns_total(J.part_out, J.nblk, s_red);
    if (threadIdx.x == 0) { J.scal[NS_S_QIN] = qin; J.scal[NS_S_QOUT] = qout; }
  }
}

// the network's own guard, and that the network result is the one this result was made over
int netsolve_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  const auto& V = h->nsv;
  const auto& W = h->net;
  if (!V.at.current(h) || !W.at.valid || W.gen != V.gen)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_netsolve_compute has been made for the map as it is now", who);
  return LBMDEM_OK;
}

int netsolve_params(const char* who, int merge, int level, int from, int band, int to, double rtol, int max_iter) {
  if (level != 0 && level != 1) return fail(LBMDEM_EINVAL, "%s: level must be 0 (between bodies) or 1 (between groups) (%d)", who, level);
  if (merge < -1) return fail(LBMDEM_EINVAL, "%s: merge must be -1 (no merging) or a difference of radii >= 0 (%d)", who, merge);
  RC_TRY(stage_check_sides(who, from, band, to, true));   // (an outlet there must be)
  if (!(rtol > 0. && rtol < 1.)) return fail(LBMDEM_EINVAL, "%s: rtol must lie strictly between 0 and 1 (%g)", who, rtol);
  if (max_iter < 0) return fail(LBMDEM_EINVAL, "%s: max_iter must not be negative, 0: the number of free regions (%d)", who, max_iter);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_netsolve_files(const char* dir, int nfile, int lx, int ly, int n, int merge, int level, int from, int band, int to,
                                const lbmdem_net_link* links, long nlinks, const lbmdem_netsolve_link* solved, long nsolved,
                                const int* region_body, long nbodies, const lbmdem_netsolve_region* regions, long nregions,
                                const long* counts10, const double* sums4, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || merge < -1 || (level != 0 && level != 1) || from < 1 || from > 15 || to < 1 || to > 15 || band < 1 || nlinks < 0 ||
      nsolved < 0 || nbodies < 0 || nregions < 0 || (nlinks > 0 && !links) || (nsolved > 0 && !solved) || (nbodies > 0 && !region_body) ||
      (nregions > 0 && !regions) || !counts10 || !sums4)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_netsolve_files arguments");
  if (lx < 2 || ly < 2 || lx > NS_SIDE_MAX || ly > NS_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_netsolve_files: the lattice is %d x %d", lx, ly);
  if (nlinks != nsolved)
    return fail(LBMDEM_EINVAL, "lbmdem_write_netsolve_files: there are %ld links in the network and %ld in the solution", nlinks, nsolved);
  if (nbodies != nregions)
    return fail(LBMDEM_EINVAL, "lbmdem_write_netsolve_files: there are %ld body numbers and %ld regions", nbodies, nregions);
  for (long k = 0; k < nregions; ++k) {
    if (region_body[k] < 0 || (k > 0 && region_body[k] <= region_body[k - 1]))
      return fail(LBMDEM_EINVAL, "lbmdem_write_netsolve_files: region %ld has the body %d: the bodies ascend from 0", k, region_body[k]);
    if (regions[k].flags < 0 || regions[k].flags > 7)
      return fail(LBMDEM_EINVAL, "lbmdem_write_netsolve_files: region %ld has the flags %d: 0 .. 7", k, regions[k].flags);
  }
  for (long k = 0; k < nlinks; ++k) {
    const lbmdem_net_link& e = links[k];
    const bool ascends = k == 0 || e.lo > links[k - 1].lo || (e.lo == links[k - 1].lo && e.hi > links[k - 1].hi);
    if (e.lo < 0 || e.lo >= e.hi || !ascends)
      return fail(LBMDEM_EINVAL, "lbmdem_write_netsolve_files: link %ld has the pair (%d, %d): the pairs ascend, 0 <= lo < hi", k, e.lo, e.hi);
  }
  OutFile F;
  RC_TRY(F.open("w", dir, "netsolve_regions%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d level %d from %d band %d to %d\n", lx, ly, n, merge, level, from, band, to);
  fprintf(fp, "# region body flags degree p net\n");
  for (long k = 0; k < nregions; ++k)
    fprintf(fp, "%ld %d %d %d %.17g %.17g\n", k, region_body[k], regions[k].flags, regions[k].degree, regions[k].p, regions[k].net);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "netsolve_links%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d level %d from %d band %d to %d\n", lx, ly, n, merge, level, from, band, to);
  fprintf(fp, "# lo hi saddle g q\n");
  for (long k = 0; k < nlinks; ++k) fprintf(fp, "%d %d %d %.17g %.17g\n", links[k].lo, links[k].hi, links[k].saddle, solved[k].g, solved[k].q);
  RC_TRY(F.close());
  return stage_append_row(F, dir, "netsolve.data",
                          "# t regions links inlet_regions outlet_regions shorted_regions free_regions iterations status flowing_links "
                          "strongest_link Q_in Q_out rz0 rz", t, counts10, LBMDEM_NETSOLVE_COUNTS, sums4, LBMDEM_NETSOLVE_SUMS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_netsolve_compute(lbmdem_handle* h, const int*, int, int, int, int, int, int, const double*, double, int, long*, double*) {
  SP_REFUSE(h, "the network pressure analysis");
}
int lbmdem_download_netsolve_regions(lbmdem_handle* h, lbmdem_netsolve_region*, long, long*) { SP_REFUSE(h, "the network pressure analysis"); }
int lbmdem_download_netsolve_links(lbmdem_handle* h, lbmdem_netsolve_link*, long, long*) { SP_REFUSE(h, "the network pressure analysis"); }
int lbmdem_netsolve_rounds(lbmdem_handle* h, int*) { SP_REFUSE(h, "the network pressure analysis"); }
int lbmdem_write_netsolve(lbmdem_handle* h, const char*, int, int, int, int, int, int, double, int) { SP_REFUSE(h, "the network pressure analysis"); }
int lbmdem_set_netsolve_output(lbmdem_handle* h, int, int, int, int, int, int, double, int) { SP_REFUSE(h, "the network pressure analysis"); }
#else

int lbmdem_netsolve_compute(lbmdem_handle* h, const int* map, int merge, int level, int from, int band, int to, int model,
                            const double* g_user, double rtol, int max_iter, long* counts10, double* sums4) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10 || !sums4) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_netsolve_compute"));
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  auto& V = h->nsv;
  V.at.valid = false;
  if (lx > NS_SIDE_MAX || ly > NS_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: a lattice of %d x %d nodes has a side above %d: the squared distances of the "
                               "network underneath are 32-bit integers", lx, ly, NS_SIDE_MAX);
  RC_TRY(netsolve_params("lbmdem_netsolve_compute", merge, level, from, band, to, rtol, max_iter));
  if (model != 0 && model != 1)
    return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: model must be 0 (plane Poiseuille from the saddle) or 1 (the caller's g) (%d)", model);
  if (model == 1 && !g_user) return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: model 1 needs g_user, one conductance per link");
  if (model == 0 && g_user) return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: g_user must be NULL with model 0");
  RC_TRY(stage_check_map("lbmdem_netsolve_compute", map, lx, ly, n));
  // the network first: the result of the handle's map is reused while its guard calls it valid and it was made with this merge
  const auto& W = h->net;
  if (map || !(W.at.current(h) && W.own && W.merge == merge)) {
    long nc[LBMDEM_NETWORK_COUNTS];
    RC_TRY(lbmdem_network_compute(h, map, merge, 0, nc));
  }
  const hipStream_t st = h->stream;
  const long B = W.nbodies, nl = W.nlinks[level], R = level ? W.ngroups : W.nbodies;
  if (R > NS_REGIONS_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: there are %ld regions, more than the %ld that three levels of the dot product's "
                               "tree hold", R, NS_REGIONS_MAX);
  if (model == 1)
    for (long k = 0; k < nl; ++k)
      if (!(g_user[k] > 0. && g_user[k] < INFINITY))
        return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: g_user[%ld] = %g: a conductance is finite and > 0", k, g_user[k]);
  const int nblk = (int)stage_blocks(R, NS_THREADS);
  const long Rc = R + R / 4 + 64, Lc = nl + nl / 4 + 64, Bc = B + B / 4 + 64, Pc = nblk + nblk / 4 + 64;
  if (!V.words) {
    HIP_TRY(h->mem.dev(&V.scal, (size_t)NS_SCAL));
    HIP_TRY(h->mem.dev(&V.words, (size_t)NS_WORDS));   // (last: the mark of a finished allocation)
  }
  HIP_TRY(h->mem.grow(&V.lints, &V.lint_cap, 7 * Lc));     // ea, eb, iota, skey, sval, cp (twice)
  HIP_TRY(h->mem.grow(&V.ldbl, &V.ldbl_cap, 4 * Lc));      // g, cg (twice), g_user
  HIP_TRY(h->mem.grow(&V.rints, &V.rint_cap, 3 * Rc));     // flo, fhi, flags
  HIP_TRY(h->mem.grow(&V.rdbl, &V.rdbl_cap, 8 * Rc));      // diag, b, x, r, z, q, d, d
  HIP_TRY(h->mem.grow(&V.bits, &V.bits_cap, Bc));
  HIP_TRY(h->mem.grow(&V.parts, &V.part_cap, 4 * Pc));
  HIP_TRY(h->mem.grow(&V.links, &V.link_cap, Lc));
  HIP_TRY(h->mem.grow(&V.regions, &V.region_cap, Rc));
  NsJob J{};
  J.lab = level ? W.group : W.body;
  J.lx = lx; J.ly = ly; J.sy = sy; J.N = (long)lx * sy;
  J.from = from; J.to = to;
  J.band = band < NS_SIDE_MAX ? band : NS_SIDE_MAX;   // (the sides are clamped to the lattice)
  J.level = level; J.model = model;
  J.B = B; J.R = R; J.L = nl;
  J.links = W.links[level]; J.bodies = W.bodies; J.groups = W.groups;
  J.ea = V.lints; J.eb = V.lints + Lc; J.iota = V.lints + 2 * Lc; J.skey = V.lints + 3 * Lc; J.sval = V.lints + 4 * Lc;
  J.cp = V.lints + 5 * Lc;
  J.g = V.ldbl; J.cg = V.ldbl + Lc; J.g_user = V.ldbl + 3 * Lc;
  J.flo = V.rints; J.fhi = V.rints + Rc; J.flags = V.rints + 2 * Rc;
  J.diag = V.rdbl; J.b = V.rdbl + Rc; J.x = V.rdbl + 2 * Rc; J.r = V.rdbl + 3 * Rc; J.z = V.rdbl + 4 * Rc; J.q = V.rdbl + 5 * Rc;
  J.d[0] = V.rdbl + 6 * Rc; J.d[1] = V.rdbl + 7 * Rc;
  J.bits = V.bits;
  J.part_dq = V.parts; J.part_rz = V.parts + Pc; J.part_in = V.parts + 2 * Pc; J.part_out = V.parts + 3 * Pc;
  J.nblk = nblk;
  J.words = V.words; J.scal = V.scal;
  J.regions = V.regions; J.out = V.links;
  J.tol2 = rtol * rtol;
  HIP_TRY(hipMemsetAsync(V.words, 0, sizeof(ns_u64) * NS_WORDS, st));
  HIP_TRY(hipMemsetAsync(V.words + NS_W_TOP_LINK, 0xFF, sizeof(ns_u64), st));   // (a minimum)
  HIP_TRY(hipMemsetAsync(V.scal, 0, sizeof(double) * NS_SCAL, st));
  HIP_TRY(hipMemsetAsync(V.bits, 0, sizeof(unsigned) * (size_t)(B > 0 ? B : 1), st));
  HIP_TRY(hipMemsetAsync(V.regions, 0, sizeof(lbmdem_netsolve_region) * (size_t)(R > 0 ? R : 1), st));
  HIP_TRY(hipMemsetAsync(J.cp, 0, sizeof(int) * 2 * (size_t)(nl > 0 ? nl : 1), st));   // (k_ns_emit fills every entry: a partner is a region whatever happens)
  HIP_TRY(hipMemsetAsync(J.cg, 0, sizeof(double) * 2 * (size_t)(nl > 0 ? nl : 1), st));
  V.rounds = 0;
  unsigned long long w[NS_WORDS] = {};
  double s[NS_SCAL] = {};
  if (R > 0) {
    if (nl > 0) {
      if (model == 1) HIP_TRY(hipMemcpyAsync(V.ldbl + 3 * Lc, g_user, sizeof(double) * (size_t)nl, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_ns_ends, dim3((unsigned)stage_blocks(nl, NS_THREADS)), dim3(NS_THREADS), 0, st, J);
      HIP_TRY(hipGetLastError());
      int bits = 1;
      while (bits < 31 && (1L << bits) < R) ++bits;
      size_t need = 0;
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, J.eb, J.skey, J.iota, J.sval, (int)nl, 0, bits, st));
      HIP_TRY(h->mem.grow(&V.tmp, &V.tmp_bytes, (long)need + 64));
      need = (size_t)V.tmp_bytes;
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(V.tmp, need, J.eb, J.skey, J.iota, J.sval, (int)nl, 0, bits, st));   // stable
    }
    hipLaunchKernelGGL(k_ns_first, dim3((unsigned)stage_blocks(R + 1, NS_THREADS)), dim3(NS_THREADS), 0, st, J);
    if (nl > 0) hipLaunchKernelGGL(k_ns_emit, dim3((unsigned)stage_blocks(nl, NS_THREADS)), dim3(NS_THREADS), 0, st, J);
    if (B > 0) hipLaunchKernelGGL(k_ns_band, dim3((unsigned)stage_blocks(J.N, NS_THREADS)), dim3(NS_THREADS), 0, st, J);
    hipLaunchKernelGGL(k_ns_flags, dim3((unsigned)nblk), dim3(NS_THREADS), 0, st, J);
    hipLaunchKernelGGL(k_ns_rows, dim3((unsigned)nblk), dim3(NS_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const long nfree = (long)w[NS_W_FREE];
    J.max_iter = max_iter > 0 ? max_iter : (int)(nfree < NS_AUTO_CAP ? nfree : NS_AUTO_CAP);
    // the iteration: launch A of iteration k makes the tests of iteration k - 1, so max_iter + 1 pairs at most
    for (long k = 1; !w[NS_W_STATUS];) {
      if (k > (long)J.max_iter + 1) return fail(LBMDEM_EINVAL, "lbmdem_netsolve_compute: the iteration did not stop in %d launches", V.rounds);
      for (int j = 0; j < NS_BATCH; ++j, ++k) {
        hipLaunchKernelGGL(k_ns_a, dim3((unsigned)nblk), dim3(NS_THREADS), 0, st, J, (int)k);
        hipLaunchKernelGGL(k_ns_b, dim3((unsigned)nblk), dim3(NS_THREADS), 0, st, J, (int)k);
        V.rounds += 2;
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(w, V.words, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    const long items = nl > R ? nl : R;
    hipLaunchKernelGGL(k_ns_out, dim3((unsigned)stage_blocks(items, NS_THREADS)), dim3(NS_THREADS), 0, st, J);
    hipLaunchKernelGGL(k_ns_last, dim3((unsigned)stage_blocks(items, NS_THREADS)), dim3(NS_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s, V.scal, sizeof s, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  } else {
    HIP_TRY(hipStreamSynchronize(st));
    w[NS_W_STATUS] = 1;
  }
  counts10[0] = R;
  counts10[1] = nl;
  counts10[2] = (long)w[NS_W_INLET];
  counts10[3] = (long)w[NS_W_OUTLET];
  counts10[4] = (long)w[NS_W_SHORTED];
  counts10[5] = (long)w[NS_W_FREE];
  counts10[6] = (long)w[NS_W_ITER];
  counts10[7] = (long)w[NS_W_STATUS] - 1;
  counts10[8] = (long)w[NS_W_FLOWING];
  counts10[9] = nl > 0 ? (long)w[NS_W_TOP_LINK] : -1;
  sums4[0] = s[NS_S_QIN]; sums4[1] = s[NS_S_QOUT]; sums4[2] = s[NS_S_RZ0]; sums4[3] = s[NS_S_LAST];
  V.nlinks = nl; V.nregions = R;
  V.gen = W.gen;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_netsolve_regions(lbmdem_handle* h, lbmdem_netsolve_region* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(netsolve_ready(h, "lbmdem_download_netsolve_regions"));
  return stage_table(h, "lbmdem_download_netsolve_regions", "regions", h->nsv.regions, sizeof *out, h->nsv.nregions, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_netsolve_links(lbmdem_handle* h, lbmdem_netsolve_link* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(netsolve_ready(h, "lbmdem_download_netsolve_links"));
  return stage_table(h, "lbmdem_download_netsolve_links", "links", h->nsv.links, sizeof *out, h->nsv.nlinks, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_netsolve_rounds(lbmdem_handle* h, int* rounds) try {
  CHECK_H(h);
  if (!rounds) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(netsolve_ready(h, "lbmdem_netsolve_rounds"));
  *rounds = h->nsv.rounds;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_netsolve(lbmdem_handle* h, const char* dir, int nfile, int merge, int level, int from, int band, int to, double rtol,
                          int max_iter) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_netsolve"));
  const LatticeView& L = h->L;
  long counts[LBMDEM_NETSOLVE_COUNTS], nl = 0, ns = 0, nr = 0, ng = 0;
  double sums[LBMDEM_NETSOLVE_SUMS];
  RC_TRY(lbmdem_netsolve_compute(h, nullptr, merge, level, from, band, to, 0, nullptr, rtol, max_iter, counts, sums));
  RC_TRY(lbmdem_download_network_links(h, level, nullptr, 0, &nl));
  RC_TRY(lbmdem_download_netsolve_links(h, nullptr, 0, &ns));
  RC_TRY(lbmdem_download_netsolve_regions(h, nullptr, 0, &nr));
  std::vector<lbmdem_net_link> links((size_t)nl);
  std::vector<lbmdem_netsolve_link> solved((size_t)ns);
  std::vector<lbmdem_netsolve_region> regions((size_t)nr);
  std::vector<int> body((size_t)nr);
  if (nl > 0) RC_TRY(lbmdem_download_network_links(h, level, links.data(), nl, &nl));
  if (ns > 0) RC_TRY(lbmdem_download_netsolve_links(h, solved.data(), ns, &ns));
  if (nr > 0) RC_TRY(lbmdem_download_netsolve_regions(h, regions.data(), nr, &nr));
  if (level == 0) {
    for (long k = 0; k < nr; ++k) body[(size_t)k] = (int)k;
  } else {
    RC_TRY(lbmdem_download_network_groups(h, nullptr, 0, &ng));
    std::vector<lbmdem_net_group> groups((size_t)ng);
    if (ng > 0) RC_TRY(lbmdem_download_network_groups(h, groups.data(), ng, &ng));
    for (long k = 0; k < nr && k < ng; ++k) body[(size_t)k] = groups[(size_t)k].body;
  }
  return lbmdem_write_netsolve_files(dir, nfile, L.lx, L.ly, h->n, merge, level, from, band, to, nl > 0 ? links.data() : nullptr, nl,
                                     ns > 0 ? solved.data() : nullptr, ns, nr > 0 ? body.data() : nullptr, nr,
                                     nr > 0 ? regions.data() : nullptr, nr, counts, sums, h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_netsolve_output(lbmdem_handle* h, int on, int merge, int level, int from, int band, int to, double rtol, int max_iter) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_netsolve_output"));
    RC_TRY(netsolve_params("lbmdem_set_netsolve_output", merge, level, from, band, to, rtol, max_iter));
    h->netsolve_merge = merge; h->netsolve_level = level;
    h->netsolve_from = from; h->netsolve_band = band; h->netsolve_to = to;
    h->netsolve_rtol = rtol; h->netsolve_max_iter = max_iter;
  }
  h->netsolve_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
