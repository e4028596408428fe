// lbm_drainage.hip -- drainage: for every fluid node the squared size of the largest disc that can be brought there from an inlet
// side without ever overlapping a solid -- the widest-path value over the clearance analysis' d2 --, per pore body and per link of
// the pore network the same, the intrusion curve and ten counts (lbmdem_drainage_compute, lbmdem_download_drainage,
// lbmdem_drainage_device, lbmdem_download_drainage_bodies, lbmdem_download_drainage_links, lbmdem_download_drainage_hist,
// lbmdem_drainage_rounds, lbmdem_write_drainage, lbmdem_set_drainage_output, lbmdem_write_drainage_files; include/lbmdem_hip.h,
// "Drainage", has the contract in full). Every result is an integer and the fixed point is unique, so nothing depends on the
// order anything happens in. Nothing here is on the step path: the kernels read the ClearanceStage's d2 and the NetworkStage's
// body plane and level-0 link table and write to the handle's DrainageStage; nothing is allocated or launched before the first
// compute.
//
// The work is done on the network, not on the grid: access[p] = min(d2[p], A[body[p]]), A per body the least fixed point of
// A[b] = max(seed[b], max over links (b, c) of min(A[c], saddle)). In the device layout (node = x*sy + y), on the handle's stream:
//   k_dr_seed     one lane per node: a fluid node of the inlet region raises A[body] to its d2 by an atomic maximum;
//   k_dr_relax    in rounds: a workgroup holds DR_CHUNK consecutive links of the table (sorted by (lo, hi): close in body number) in
//                 registers and sweeps them -- atomicMax(A[lo], min(A[hi], saddle)) and the same with the ends swapped -- until
//                 DR_LINGER sweeps in a row changed nothing, DR_SWEEPS at most. Values only rise, and only to values a real path
//                 realises, so any order ends at the same fixed point. A launch that raised something raises `changed`; the host
//                 stops at the first quiet launch, in which every link was evaluated over an A that nothing changed. A launch with
//                 a change finishes at least the highest body not yet final: bodies + 1 launches at most. No workgroup waits for
//                 another; A is read and written through relaxed agent-scope atomics only;
//   k_dr_plane    lanes along y, DR_ROWS rows per workgroup: the access plane (0 in the pad columns), the histogram of
//                 isqrt(access) (the lanes of a wavefront that share a bin first, LDS bins, then 64-bit atomics), the node counts,
//                 the largest access, and over the outlet the maximum of access << 32 | ~k: critical and critical_node;
//   k_dr_tables   one lane per body and link: the reached bodies, pass, the front links (critical is there by now).
// Integer atomics only, no floating point anywhere. Every loop has the bound its comment states.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both. Front end, as every export's: whole_handle(), SP_REFUSE() (lbmdem_handle.h), MemPool (lbm_mem.h), OutFile (lbm_outfile.h),
// lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>

namespace {

constexpr int DR_SIDE_MAX = 32768;   // the clearance analysis': d2 < 2^31, a node's index < 2^30

#ifndef LBMDEM_SINGLE_PRECISION
typedef unsigned long long dr_u64;
constexpr int DR_THREADS = 256;
constexpr int DR_ROWS = 32;          // rows per workgroup of the plane pass
constexpr int DR_PER = 1;            // links per lane of the relaxation
constexpr int DR_CHUNK = DR_THREADS * DR_PER;
constexpr int DR_LINGER = 32;        // quiet sweeps after which a workgroup leaves: values from other chunks may still arrive
constexpr int DR_SWEEPS = 4096;      // sweeps per workgroup and launch at most
constexpr int DR_LDS_BINS = 2048;    // histogram bins a workgroup keeps in LDS; the bins beyond go to global memory at once
// DrainageStage::words
enum : int { DR_W_FLUID = 0, DR_W_INLET, DR_W_REACHED, DR_W_SHIELDED, DR_W_OUTLET, DR_W_MAX, DR_W_CRIT, DR_W_BODIES, DR_W_FRONT,
             DR_W_CHANGED, DR_WORDS };
constexpr int DR_PLANE_WORDS = DR_W_CRIT + 1;   // the words the plane pass makes: sums up to DR_W_OUTLET, then two maxima

struct DrJob {
  const int* d2;     // [lx][sy] the clearance analysis' plane: > 0 exactly on the fluid, 0 in the pad columns
  const int* body;   // [lx][sy] the network's: the body's number, -1 off the fluid and in the pad columns
  int lx, ly, sy;
  long N;            // lx * sy
  int from, to, band;
  int* A;            // [B]
  long B;
  const lbmdem_net_link* links;   // [L] level 0, ascending (lo, hi)
  long L;
  int* pass;         // [L]
  int* access;       // [lx][sy]
  dr_u64* hist;      // [hbins]
  int hbins;
  dr_u64* words;
};

__device__ __forceinline__ int dr_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dr_raise(int* p, int v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the region of a side mask: B 1 (y low), T 2 (y high), L 4 (x low), R 8 (x high), `band` nodes deep (band >= 1)
__device__ __forceinline__ bool dr_region(const DrJob& J, int mask, int x, int y) {
  return ((mask & 1) && y < J.band) || ((mask & 2) && y >= J.ly - J.band) || ((mask & 4) && x < J.band) || ((mask & 8) && x >= J.lx - J.band);
}

__global__ __launch_bounds__(DR_THREADS) void k_dr_seed(const DrJob J) {
  const long node = (long)blockIdx.x * DR_THREADS + threadIdx.x;
  if (node >= J.N) return;
  const int x = (int)(node / J.sy), y = (int)(node % J.sy);
  if (y >= J.ly || !dr_region(J, J.from, x, y)) return;
  const int d = J.d2[node];
  if (d <= 0) return;
  const int b = J.body[node];
  if (b < 0 || b >= J.B) return;   // (never: a fluid node has a body)
  if (dr_load(J.A + b) < d) dr_raise(J.A + b, d);
}

__global__ __launch_bounds__(DR_THREADS) void k_dr_relax(const DrJob J) {
  int lo[DR_PER], hi[DR_PER], sd[DR_PER];
#pragma unroll
  for (int k = 0; k < DR_PER; ++k) {
    const long t = (long)blockIdx.x * DR_CHUNK + k * DR_THREADS + threadIdx.x;
    lo[k] = hi[k] = 0;
    sd[k] = 0;   // (0: no link here; a saddle is >= 1)
    if (t < J.L) {
      const lbmdem_net_link e = J.links[t];
      if (e.lo >= 0 && e.lo < J.B && e.hi >= 0 && e.hi < J.B) { lo[k] = e.lo; hi[k] = e.hi; sd[k] = e.saddle; }   // (always)
    }
  }
  int any = 0, quiet = 0;
  for (int sweep = 0; sweep < DR_SWEEPS; ++sweep) {
    int ch = 0;
#pragma unroll
    for (int k = 0; k < DR_PER; ++k) {
      if (sd[k] <= 0) continue;
      int a = dr_load(J.A + lo[k]);
      const int b = dr_load(J.A + hi[k]);
      const int va = b < sd[k] ? b : sd[k];
      if (va > a) { dr_raise(J.A + lo[k], va); a = va; ch = 1; }
      const int vb = a < sd[k] ? a : sd[k];
      if (vb > b) { dr_raise(J.A + hi[k], vb); ch = 1; }
    }
    any |= ch;
    quiet = __syncthreads_or(ch) ? 0 : quiet + 1;   // (the same number in every lane)
    if (quiet >= DR_LINGER) break;
  }
  if (any) __hip_atomic_store(J.words + DR_W_CHANGED, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// floor(sqrt(v)) in integers, 16 rounds
__device__ __forceinline__ int dr_isqrt(unsigned v) {
  unsigned r = 0;
#pragma unroll
  for (unsigned b = 1u << 15; b; b >>= 1) {
    const unsigned t = r | b;
    if (t * t <= v) r = t;
  }
  return (int)r;
}

__device__ __forceinline__ dr_u64 dr_wave_sum(dr_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}
__device__ __forceinline__ dr_u64 dr_wave_max(dr_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) { const dr_u64 o = __shfl_xor(v, m); v = o > v ? o : v; }
  return v;
}

__global__ __launch_bounds__(DR_THREADS) void k_dr_plane(const DrJob J) {
  __shared__ unsigned s_hist[DR_LDS_BINS];
  __shared__ dr_u64 s_w[DR_PLANE_WORDS];
  for (int i = threadIdx.x; i < DR_LDS_BINS; i += DR_THREADS) s_hist[i] = 0;
  if (threadIdx.x < DR_PLANE_WORDS) s_w[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * DR_THREADS + threadIdx.x;
  const int lx = J.lx, ly = J.ly, sy = J.sy;
  const bool inside = y < ly;
  dr_u64 w[DR_PLANE_WORDS] = {};   // this lane's, over its rows
  for (int r = 0; r < DR_ROWS; ++r) {
    const int x = blockIdx.y * DR_ROWS + r;
    if (x >= lx) break;   // (the whole workgroup)
    const long node = (long)x * sy + y;
    int d = 0, a = 0;
    if (inside) {
      d = J.d2[node];
      if (d > 0) {
        const int b = J.body[node];
        const int ab = b >= 0 && b < J.B ? J.A[b] : 0;   // (always a body)
        a = d < ab ? d : ab;
      }
    }
    if (y < sy) J.access[node] = a;   // (the pad columns: 0)
    const bool fluid = d > 0;
    if (fluid) {
      w[DR_W_FLUID] += 1;
      w[DR_W_INLET] += dr_region(J, J.from, x, y);
      w[DR_W_REACHED] += a > 0;
      w[DR_W_SHIELDED] += a > 0 && a < d;
      if ((dr_u64)(unsigned)a > w[DR_W_MAX]) w[DR_W_MAX] = (dr_u64)(unsigned)a;
      if (dr_region(J, J.to, x, y)) {
        w[DR_W_OUTLET] += 1;
        const dr_u64 mine = (dr_u64)(unsigned)a << 32 | (dr_u64)(0xFFFFFFFFu - (unsigned)((long)x * ly + y));   // the smaller index wins
        if (a > 0 && mine > w[DR_W_CRIT]) w[DR_W_CRIT] = mine;
      }
    }
    // the lanes that share a bin: every round retires its leader's lanes, 64 rounds at most
    const int k = dr_isqrt((unsigned)a);
    dr_u64 todo = __ballot(fluid);
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int kk = __shfl(k, lead);
      const dr_u64 same = __ballot(fluid && k == kk);
      if (lane == lead) {
        if (kk < DR_LDS_BINS) atomicAdd(&s_hist[kk], (unsigned)__popcll(same));
        else if (kk < J.hbins) atomicAdd(&J.hist[kk], (dr_u64)__popcll(same));
      }
      todo &= ~same;
    }
  }
#pragma unroll
  for (int i = 0; i < DR_PLANE_WORDS; ++i) {
    const dr_u64 v = i < DR_W_MAX ? dr_wave_sum(w[i]) : dr_wave_max(w[i]);
    if (lane == 0 && v) { if (i < DR_W_MAX) atomicAdd(&s_w[i], v); else atomicMax(&s_w[i], v); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DR_LDS_BINS && i < J.hbins; i += DR_THREADS)
    if (s_hist[i]) atomicAdd(&J.hist[i], (dr_u64)s_hist[i]);
  if (threadIdx.x < DR_PLANE_WORDS && s_w[threadIdx.x]) {
    if (threadIdx.x < DR_W_MAX) atomicAdd(&J.words[threadIdx.x], s_w[threadIdx.x]);
    else atomicMax(&J.words[threadIdx.x], s_w[threadIdx.x]);
  }
}

__global__ __launch_bounds__(DR_THREADS) void k_dr_tables(const DrJob J) {
  const long i = (long)blockIdx.x * DR_THREADS + threadIdx.x;
  const int critical = (int)(J.words[DR_W_CRIT] >> 32);   // (k_dr_plane has finished)
  bool reached = false, front = false;
  if (i < J.B) reached = J.A[i] > 0;
  if (i < J.L) {
    const lbmdem_net_link e = J.links[i];
    int p = 0;
    if (e.lo >= 0 && e.lo < J.B && e.hi >= 0 && e.hi < J.B) {   // (always)
      const int a = J.A[e.lo], b = J.A[e.hi];
      const int low = a < b ? a : b, high = a < b ? b : a;
      p = low < e.saddle ? low : e.saddle;
      front = critical > 0 && e.saddle == critical && high > critical && low == critical;
    }
    J.pass[i] = p;
  }
  const dr_u64 nreached = __popcll(__ballot(reached)), nfront = __popcll(__ballot(front));
  if ((threadIdx.x & 63) == 0) {
    if (nreached) atomicAdd(&J.words[DR_W_BODIES], nreached);
    if (nfront) atomicAdd(&J.words[DR_W_FRONT], nfront);
  }
}

// what depends on the lattice, once (the clearance stage, whose bin count this one shares, is there: a network compute has run)
int drainage_stage(lbmdem_handle* h) {
  auto& V = h->drn;
  if (V.words) return LBMDEM_OK;
  const size_t N = (size_t)h->L.lx * h->L.sy;
  HIP_TRY(h->mem.dev(&V.access, N));
  HIP_TRY(h->mem.dev(&V.hist, (size_t)h->clr.hbins));
  HIP_TRY(h->mem.dev(&V.words, (size_t)DR_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

// the network's own guard, and that the network result is the one this drainage result was made over
int drainage_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  const auto& V = h->drn;
  const auto& W = h->net;
  if (!V.at.current(h) || !W.at.valid || W.gen != V.gen)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_drainage_compute has been made for the map as it is now", who);
  return LBMDEM_OK;
}

#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_drainage_files(const char* dir, int nfile, int lx, int ly, int n, int from, int band, int to, int plane,
                                const int* access, const lbmdem_net_body* bodies, long nbodies, const int* A, long nA,
                                const long* hist, long nhist, const long* clearance_hist, long nclearance_hist,
                                const long* counts10, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || nbodies < 0 || nA < 0 || (nbodies > 0 && !bodies) || (nA > 0 && !A) || nhist < 1 || !hist || nclearance_hist < 1 ||
      !clearance_hist || !counts10 || (plane && !access) || from < 1 || from > 15 || to < 0 || to > 15 || band < 1)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_drainage_files arguments");
  if (lx < 2 || ly < 2 || lx > DR_SIDE_MAX || ly > DR_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: the lattice is %d x %d", lx, ly);
  if (nA != nbodies)
    return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: there are %ld bodies and %ld values of A", nbodies, nA);
  if (nhist != nclearance_hist)
    return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: the access histogram has %ld bins, the clearance histogram %ld", nhist,
                nclearance_hist);
  const long cnt = (long)lx * ly;
  for (long k = 0; k < nbodies; ++k) {
    const lbmdem_net_body& e = bodies[k];
    if (e.d2 < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: body %ld has the negative d2 %d", k, e.d2);
    if (e.node < 0 || e.node >= cnt || (k > 0 && e.node <= bodies[k - 1].node))
      return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: body %ld has the node %d: the nodes ascend, 0 <= node < %ld", k, e.node, cnt);
    if (A[k] < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: body %ld has the negative A %d", k, A[k]);
    if (A[k] > e.d2) return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: body %ld has A = %d above its d2 = %d", k, A[k], e.d2);
  }
  for (long k = 0; k < nhist; ++k)
    if (hist[k] < 0 || clearance_hist[k] < 0)
      return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: bin %ld holds %ld and %ld nodes: a count is not negative", k, hist[k],
                  clearance_hist[k]);
  if (plane)
    for (long k = 0; k < cnt; ++k)
      if (access[k] < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_drainage_files: access[%ld][%ld] = %d is negative", k / ly, k % ly, access[k]);
  OutFile F;
  RC_TRY(F.open("w", dir, "drainage_curve%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d from %d band %d to %d\n", lx, ly, n, from, band, to);
  fprintf(fp, "# k access_nodes clearance_nodes invaded\n");
  {
    std::vector<long> invaded((size_t)nhist + 1, 0);   // nodes with isqrt(access) >= max(k, 1)
    for (long k = nhist - 1; k >= 1; --k) invaded[(size_t)k] = invaded[(size_t)k + 1] + hist[k];
    invaded[0] = nhist > 1 ? invaded[1] : 0;
    for (long k = 0; k < nhist; ++k) fprintf(fp, "%ld %ld %ld %ld\n", k, hist[k], clearance_hist[k], invaded[(size_t)k]);
  }
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "drainage_bodies%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d from %d band %d to %d\n", lx, ly, n, from, band, to);
  fprintf(fp, "# body node d2 A\n");
  for (long k = 0; k < nbodies; ++k) fprintf(fp, "%ld %d %d %d\n", k, bodies[k].node, bodies[k].d2, A[k]);
  RC_TRY(F.close());
  if (plane) {
    const char* const names[1] = {"access"};
    RC_TRY(stage_write_int_planes(F, dir, nfile, "drainage%.6i.vtk", "lbmdem drainage", lx, ly, names, &access, 1));
  }
  return stage_append_row(F, dir, "drainage.data",
                          "# t fluid_nodes inlet_nodes reached_nodes reached_bodies access_max shielded_nodes outlet_nodes critical "
                          "critical_node front_links", t, counts10, LBMDEM_DRAINAGE_COUNTS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_drainage_compute(lbmdem_handle* h, const int*, int, int, int, long, long*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_download_drainage(lbmdem_handle* h, int*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_drainage_device(lbmdem_handle* h, const int**, int*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_download_drainage_bodies(lbmdem_handle* h, int*, long, long*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_download_drainage_links(lbmdem_handle* h, int*, long, long*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_download_drainage_hist(lbmdem_handle* h, long*, long, long*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_drainage_rounds(lbmdem_handle* h, int*) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_write_drainage(lbmdem_handle* h, const char*, int, int, int, int, int) { SP_REFUSE(h, "the drainage analysis"); }
int lbmdem_set_drainage_output(lbmdem_handle* h, int, int, int, int, int) { SP_REFUSE(h, "the drainage analysis"); }
#else

int lbmdem_drainage_compute(lbmdem_handle* h, const int* map, int from, int band, int to, long max_edges, long* counts10) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_drainage_compute"));
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  auto& V = h->drn;
  V.at.valid = false;
  if (lx > DR_SIDE_MAX || ly > DR_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_drainage_compute: a lattice of %d x %d nodes has a side above %d: the squared distances are "
                               "32-bit integers", lx, ly, DR_SIDE_MAX);
  RC_TRY(stage_check_sides("lbmdem_drainage_compute", from, band, to));
  RC_TRY(stage_check_max_edges("lbmdem_drainage_compute", max_edges));
  RC_TRY(stage_check_map("lbmdem_drainage_compute", map, lx, ly, n));
  // the network first: the result of the handle's map is reused while its guard calls it valid and the d2 it was made over is there
  const auto& Q = h->clr;
  const auto& W = h->net;
  if (map || !(Q.at.current(h) && Q.own) || !(W.at.current(h) && W.own)) {
    long nc[LBMDEM_NETWORK_COUNTS];
    RC_TRY(lbmdem_network_compute(h, map, -1, max_edges, nc));
  }
  RC_TRY(drainage_stage(h));
  const hipStream_t st = h->stream;
  const long B = W.nbodies, nl = W.nlinks[0];
  HIP_TRY(h->mem.grow(&V.A, &V.a_cap, B + B / 4 + 64));
  HIP_TRY(h->mem.grow(&V.pass, &V.pass_cap, nl + nl / 4 + 64));
  DrJob J{};
  J.d2 = Q.d2; J.body = W.body;
  J.lx = lx; J.ly = ly; J.sy = sy;
  J.N = (long)lx * sy;
  J.from = from; J.to = to;
  J.band = band < DR_SIDE_MAX ? band : DR_SIDE_MAX;   // (the sides are clamped to the lattice)
  J.A = V.A; J.B = B;
  J.links = W.links[0]; J.L = nl;
  J.pass = V.pass;
  J.access = V.access;
  J.hist = V.hist; J.hbins = Q.hbins;
  J.words = V.words;
  HIP_TRY(hipMemsetAsync(V.words, 0, sizeof(dr_u64) * DR_WORDS, st));
  HIP_TRY(hipMemsetAsync(V.hist, 0, sizeof(dr_u64) * (size_t)Q.hbins, st));
  HIP_TRY(hipMemsetAsync(V.A, 0, sizeof(int) * (size_t)(B > 0 ? B : 1), st));
  if (B > 0) hipLaunchKernelGGL(k_dr_seed, dim3((unsigned)stage_blocks(J.N, DR_THREADS)), dim3(DR_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  // the relaxation: until a launch raises nothing
  V.rounds = 0;
  for (long round = 1; nl > 0; ++round) {
    if (round > B + 1) return fail(LBMDEM_EINVAL, "lbmdem_drainage_compute: the relaxation did not settle in %ld rounds", B + 1);
    HIP_TRY(hipMemsetAsync(V.words + DR_W_CHANGED, 0, sizeof(dr_u64), st));
    hipLaunchKernelGGL(k_dr_relax, dim3((unsigned)stage_blocks(nl, DR_CHUNK)), dim3(DR_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    unsigned long long changed = 0;
    HIP_TRY(hipMemcpyAsync(&changed, V.words + DR_W_CHANGED, sizeof changed, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    V.rounds = (int)round;
    if (!changed) break;
  }
  hipLaunchKernelGGL(k_dr_plane, dim3((unsigned)stage_blocks(sy, DR_THREADS), (unsigned)stage_blocks(lx, DR_ROWS)), dim3(DR_THREADS), 0, st, J);
  const long items = B > nl ? B : nl;
  if (items > 0) hipLaunchKernelGGL(k_dr_tables, dim3((unsigned)stage_blocks(items, DR_THREADS)), dim3(DR_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[DR_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts10[0] = (long)w[DR_W_FLUID];
  counts10[1] = (long)w[DR_W_INLET];
  counts10[2] = (long)w[DR_W_REACHED];
  counts10[3] = (long)w[DR_W_BODIES];
  counts10[4] = (long)w[DR_W_MAX];
  counts10[5] = (long)w[DR_W_SHIELDED];
  counts10[6] = (long)w[DR_W_OUTLET];
  counts10[7] = to == 0 ? -1 : (long)(w[DR_W_CRIT] >> 32);
  counts10[8] = w[DR_W_CRIT] ? (long)(0xFFFFFFFFu - (unsigned)w[DR_W_CRIT]) : -1;
  counts10[9] = (long)w[DR_W_FRONT];
  V.nbodies = B; V.nlinks = nl; V.kmax = Q.kmax;
  V.gen = W.gen;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_drainage(lbmdem_handle* h, int* access) try {
  CHECK_H(h);
  if (!access) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(drainage_ready(h, "lbmdem_download_drainage"));
  RC_TRY(stage_download_plane(h, access, h->drn.access));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_drainage_device(lbmdem_handle* h, const int** access, int* sy) try {
  CHECK_H(h);
  if (!access || !sy) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(drainage_ready(h, "lbmdem_drainage_device"));
  *access = h->drn.access;
  *sy = h->L.sy;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_drainage_bodies(lbmdem_handle* h, int* A, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !A)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(drainage_ready(h, "lbmdem_download_drainage_bodies"));
  return stage_table(h, "lbmdem_download_drainage_bodies", "bodies", h->drn.A, sizeof *A, h->drn.nbodies, A, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_drainage_links(lbmdem_handle* h, int* pass, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !pass)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(drainage_ready(h, "lbmdem_download_drainage_links"));
  return stage_table(h, "lbmdem_download_drainage_links", "links", h->drn.pass, sizeof *pass, h->drn.nlinks, pass, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_drainage_hist(lbmdem_handle* h, long* hist, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !hist)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(drainage_ready(h, "lbmdem_download_drainage_hist"));
  return stage_table(h, "lbmdem_download_drainage_hist", "bins", h->drn.hist, sizeof *hist, (long)h->drn.kmax + 1, hist, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_drainage_rounds(lbmdem_handle* h, int* rounds) try {
  CHECK_H(h);
  if (!rounds) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(drainage_ready(h, "lbmdem_drainage_rounds"));
  *rounds = h->drn.rounds;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_drainage(lbmdem_handle* h, const char* dir, int nfile, int from, int band, int to, int plane) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_drainage"));
  const LatticeView& L = h->L;
  long counts[LBMDEM_DRAINAGE_COUNTS], nb = 0, na = 0, nh = 0, nc = 0;
  RC_TRY(lbmdem_drainage_compute(h, nullptr, from, band, to, 0, counts));
  RC_TRY(lbmdem_download_network_bodies(h, nullptr, 0, &nb));
  RC_TRY(lbmdem_download_drainage_bodies(h, nullptr, 0, &na));
  RC_TRY(lbmdem_download_drainage_hist(h, nullptr, 0, &nh));
  RC_TRY(lbmdem_download_clearance_hist(h, nullptr, 0, &nc));
  std::vector<lbmdem_net_body> bodies((size_t)nb);
  std::vector<int> A((size_t)na), access;
  std::vector<long> hist((size_t)nh), chist((size_t)nc);
  if (nb > 0) RC_TRY(lbmdem_download_network_bodies(h, bodies.data(), nb, &nb));
  if (na > 0) RC_TRY(lbmdem_download_drainage_bodies(h, A.data(), na, &na));
  RC_TRY(lbmdem_download_drainage_hist(h, hist.data(), nh, &nh));
  RC_TRY(lbmdem_download_clearance_hist(h, chist.data(), nc, &nc));
  if (plane) {
    access.resize((size_t)L.lx * L.ly);
    RC_TRY(lbmdem_download_drainage(h, access.data()));
  }
  return lbmdem_write_drainage_files(dir, nfile, L.lx, L.ly, h->n, from, band, to, plane, plane ? access.data() : nullptr,
                                     nb > 0 ? bodies.data() : nullptr, nb, na > 0 ? A.data() : nullptr, na, hist.data(), nh,
                                     chist.data(), nc, counts, h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_drainage_output(lbmdem_handle* h, int on, int from, int band, int to, int plane) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_drainage_output"));
    RC_TRY(stage_check_sides("lbmdem_set_drainage_output", from, band, to));
    h->drainage_from = from; h->drainage_band = band; h->drainage_to = to;
    h->drainage_plane = plane != 0;
  }
  h->drainage_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
