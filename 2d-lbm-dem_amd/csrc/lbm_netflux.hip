// lbm_netflux.hip -- pore fluxes: the mass that crossed every edge of adjacent fluid nodes in the last streaming step, in fixed
// point, summed per link and per region of the pore network and per section of the lattice (lbmdem_netflux_compute,
// lbmdem_download_netflux_links, lbmdem_download_netflux_regions, lbmdem_download_netflux_profile, lbmdem_write_netflux,
// lbmdem_set_netflux_output, lbmdem_write_netflux_files; include/lbmdem_hip.h, "Pore fluxes", has the contract in full). Every
// addend is rint(x * 2^32) in a wrapping 64-bit integer, so no sum depends on the order anything happens in. Nothing here is on
// the step path: the kernels read f, the NetworkStage's label plane of the level (body or group: >= 0 exactly on the fluid of the
// map the network was made over, so the map itself is not read again) and its link table, and write to the handle's NetfluxStage;
// nothing is allocated or launched before the first compute.
//
// In the device layout (node = x*sy + y), on the handle's stream, single launches:
//   k_nf_first    one lane per body number b: first[b], the first link with lo >= b (a binary search of the table, which ascends by
//                 (lo, hi)); first[b] .. first[b + 1] is b's run, in which an edge finds its link by a binary search over hi;
//   k_nf_plane    a workgroup owns 256 columns (lanes along y) and NF_ROWS rows and marches along x with the row in front in
//                 registers: a node's label and nine populations are read once per workgroup (a segment's first row twice), y -+ 1
//                 comes from the neighbouring lanes, the first and the last lane of a wave read one halo column each. Per node rho
//                 and the Q of its four forward edges; row[y] in two registers per lane over the rows and one atomic per lane at
//                 the end (lane 0 of a wave one more); col[x] by a wavefront sum, one atomic per wave and row; the mass per region
//                 as runs of one label along the lanes, an LDS slot per label modulo 64, then 64-bit atomics; a ridge edge adds Q,
//                 |Q| and 1 to its link, the edges of one node that cross to the same region together;
//   k_nf_tables   one lane per link: net and through into its two regions, flowing_links, the atomic maximum of |flux|;
//   k_nf_regions  one lane per link and region: the atomic minimum of the index among the links that hold that maximum; the region
//                 records in the order of the level's table, the largest |net|.
// The per-region sums are kept by body number (a group's number is its root body's), so no table from a root to its group's place
// is needed: k_nf_regions reads the place's body from the group table. Integer atomics only. Every loop has the bound its comment
// states.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both. Front end, as every export's: whole_handle(), SP_REFUSE() (lbmdem_handle.h), MemPool (lbm_mem.h), OutFile (lbm_outfile.h),
// lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>

namespace {

constexpr int NF_SIDE_MAX = 32768;   // the clearance analysis': a node's index < 2^30

#ifndef LBMDEM_SINGLE_PRECISION
typedef unsigned long long nf_u64;
constexpr int NF_THREADS = 256;
constexpr int NF_ROWS = 32;          // rows per workgroup of the plane pass
constexpr int NF_SLOTS = 64;         // LDS slots of the regions' masses, by label modulo NF_SLOTS
constexpr double NF_Q32 = 4294967296.;
constexpr double NF_MAX = 1048576.;  // 2^20: the pore table's rule for mass_q32
// NetfluxStage::words
enum : int { NF_W_FLUID = 0, NF_W_EDGES, NF_W_RIDGE, NF_W_BAD_EDGES, NF_W_BAD_NODES, NF_W_FLOWING, NF_W_TOP, NF_W_TOP_LINK, NF_W_IMBALANCE,
             NF_WORDS };
constexpr int NF_PLANE_WORDS = NF_W_BAD_NODES + 1;   // the words the plane pass makes, all sums

struct NfJob {
  const real* f;
  const int* lab;    // [lx][sy] the network's body or group plane: a body's number, -1 off the fluid and in the pad columns
  int lx, ly, sy;
  long B;            // body numbers: 0 .. B - 1 at either level
  const lbmdem_net_link* links;   // [L] of the level, ascending (lo, hi)
  long L;
  int* first;        // [B + 1]
  nf_u64* mass;      // [B] by body number
  nf_u64* net;       // [B]
  nf_u64* through;   // [B]
  lbmdem_netflux_link* out;   // [L]
  nf_u64* col;       // [lx]: lx - 1 sections
  nf_u64* row;       // [ly]: ly - 1 sections
  nf_u64* words;
  const lbmdem_net_group* groups;   // level 1: [R]
  long R;
  int level;
  lbmdem_netflux_region* regions;   // [R]
};

__global__ __launch_bounds__(NF_THREADS) void k_nf_first(const NfJob J) {
  const long b = (long)blockIdx.x * NF_THREADS + threadIdx.x;
  if (b > J.B) return;
  long a = 0, e = J.L;   // the first link with lo >= b: at most 32 halvings
  while (a < e) {
    const long m = (a + e) >> 1;
    if ((long)J.links[m].lo < b) a = m + 1; else e = m;
  }
  J.first[b] = (int)a;
}

// the link (lo, hi), lo < hi < B: a binary search over hi in lo's run, at most 32 halvings; -1 if there is none (never)
__device__ __forceinline__ long nf_find(const NfJob& J, int lo, int hi) {
  long a = J.first[lo], e = J.first[lo + 1];
  if (a < 0 || e > J.L) return -1;   // (never)
  while (a < e) {
    const long m = (a + e) >> 1;
    if (J.links[m].hi < hi) a = m + 1; else e = m;
  }
  return a < J.L && J.links[a].lo == lo && J.links[a].hi == hi ? a : -1;
}

// rint(x * 2^32), or 0 with *bad raised when x is not finite or |x| >= 2^20 (the comparison is false for a NaN)
__device__ __forceinline__ long long nf_q32(double x, int* bad) {
  if (fabs(x) < NF_MAX) return __double2ll_rn(x * NF_Q32);
  ++*bad;
  return 0;
}

__device__ __forceinline__ nf_u64 nf_abs(long long v) { return v < 0 ? 0ull - (nf_u64)v : (nf_u64)v; }

__device__ __forceinline__ nf_u64 nf_wave_sum(nf_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}

// a lattice row as the march keeps it: the lane's label and populations, and of its two neighbours in y what the edges need
struct NfRow {
  double f[9];
  double f5m, f7p, f8p;   // direction 5 of (x, y - 1), 7 and 8 of (x, y + 1)
  int lab, labm, labp;    // of (x, y), (x, y - 1), (x, y + 1); -1: no fluid node there
};

__device__ __forceinline__ int nf_label(const NfJob& J, int x, int y) {
  if (x < 0 || x >= J.lx || y < 0 || y >= J.ly) return -1;
  const int l = J.lab[(long)x * J.sy + y];
  return l >= 0 && l < J.B ? l : -1;   // (never beyond B)
}

// (every lane of the wavefront comes here together: wave shifts)
__device__ __forceinline__ NfRow nf_row(const NfJob& J, int x, int y, int lane) {
  NfRow R;
#pragma unroll
  for (int q = 0; q < 9; ++q) R.f[q] = 0.;
  R.lab = nf_label(J, x, y);
  if (R.lab >= 0) {
    const long fb = fbase((long)x * J.sy + y);
#pragma unroll
    for (int q = 0; q < 9; ++q) R.f[q] = J.f[fb + q * LBMDEM_TILE_Y];
  }
  int hl = -1;
  double h5 = 0., h7 = 0., h8 = 0.;
  if (lane == 0 || lane == 63) {   // the halo column of a wave's first and last lane
    const int yh = lane == 0 ? y - 1 : y + 1;
    hl = nf_label(J, x, yh);
    if (hl >= 0) {
      const long fb = fbase((long)x * J.sy + yh);
      if (lane == 0) h5 = J.f[fb + 5 * LBMDEM_TILE_Y];
      else { h7 = J.f[fb + 7 * LBMDEM_TILE_Y]; h8 = J.f[fb + 8 * LBMDEM_TILE_Y]; }
    }
  }
  R.labm = __shfl_up(R.lab, 1); R.f5m = __shfl_up(R.f[5], 1);
  R.labp = __shfl_down(R.lab, 1); R.f7p = __shfl_down(R.f[7], 1); R.f8p = __shfl_down(R.f[8], 1);
  if (lane == 0) { R.labm = hl; R.f5m = h5; }
  if (lane == 63) { R.labp = hl; R.f7p = h7; R.f8p = h8; }
  return R;
}

// what the edges of one node towards one other region add to that link
__device__ __forceinline__ void nf_link_add(const NfJob& J, int mine, int other, long long q, nf_u64 aq, int n) {
  const int lo = mine < other ? mine : other, hi = mine < other ? other : mine;
  const long t = nf_find(J, lo, hi);
  if (t < 0) return;   // (never: the network has a link for every pair of adjacent regions)
  lbmdem_netflux_link* e = J.out + t;
  const long long fx = mine == lo ? q : -q;
  if (fx) atomicAdd(reinterpret_cast<nf_u64*>(&e->flux_q32), (nf_u64)fx);
  if (aq) atomicAdd(reinterpret_cast<nf_u64*>(&e->exchange_q32), aq);
  atomicAdd(reinterpret_cast<nf_u64*>(&e->edges), (nf_u64)n);
}

__global__ __launch_bounds__(NF_THREADS) void k_nf_plane(const NfJob J) {
  __shared__ int s_lab[NF_SLOTS];
  __shared__ nf_u64 s_mass[NF_SLOTS];
  __shared__ nf_u64 s_w[NF_PLANE_WORDS];
  if (threadIdx.x < NF_SLOTS) { s_lab[threadIdx.x] = -1; s_mass[threadIdx.x] = 0; }
  if (threadIdx.x < NF_PLANE_WORDS) s_w[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * NF_THREADS + threadIdx.x;
  const int lx = J.lx, ly = J.ly;
  const int xa = blockIdx.y * NF_ROWS;
  const int xb = xa + NF_ROWS < lx ? xa + NF_ROWS : lx;
  nf_u64 w[NF_PLANE_WORDS] = {};   // this lane's, over its rows
  nf_u64 row_here = 0, row_below = 0;   // towards row[y] and row[y - 1]
  NfRow cur = nf_row(J, xa, y, lane);
  for (int x = xa; x < xb; ++x) {   // (every lane stays in the loop: wave shifts)
    const NfRow nx = nf_row(J, x + 1, y, lane);   // (beyond the lattice: no fluid)
    const bool fluid = cur.lab >= 0;
    long long mass = 0, q[4] = {0, 0, 0, 0};
    int other[4] = {-1, -1, -1, -1};   // the edges towards (x, y + 1), (x + 1, y - 1), (x + 1, y), (x + 1, y + 1): directions 8, 5, 6, 7
    if (fluid) {
      int bad = 0;
      const double rho = cur.f[0] + cur.f[1] + cur.f[2] + cur.f[3] + cur.f[4] + cur.f[5] + cur.f[6] + cur.f[7] + cur.f[8];
      mass = nf_q32(rho, &bad);
      w[NF_W_FLUID] += 1;
      w[NF_W_BAD_NODES] += (nf_u64)bad;
      bad = 0;
      other[0] = cur.labp; other[1] = nx.labm; other[2] = nx.lab; other[3] = nx.labp;
      if (other[0] >= 0) q[0] = nf_q32(cur.f8p - cur.f[4], &bad);
      if (other[1] >= 0) q[1] = nf_q32(nx.f5m - cur.f[1], &bad);
      if (other[2] >= 0) q[2] = nf_q32(nx.f[6] - cur.f[2], &bad);
      if (other[3] >= 0) q[3] = nf_q32(nx.f7p - cur.f[3], &bad);
      w[NF_W_BAD_EDGES] += (nf_u64)bad;
      w[NF_W_EDGES] += (nf_u64)((other[0] >= 0) + (other[1] >= 0) + (other[2] >= 0) + (other[3] >= 0));
      row_here += (nf_u64)q[0] + (nf_u64)q[3];
      row_below -= (nf_u64)q[1];
      // the ridge edges, those towards one region together: four edges at most
      int to = -1, n = 0;
      long long sq = 0;
      nf_u64 sa = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (other[k] < 0 || other[k] == cur.lab) continue;
        if (other[k] != to) {
          if (n) nf_link_add(J, cur.lab, to, sq, sa, n);
          to = other[k]; n = 0; sq = 0; sa = 0;
        }
        ++n; sq += q[k]; sa += nf_abs(q[k]);
        w[NF_W_RIDGE] += 1;
      }
      if (n) nf_link_add(J, cur.lab, to, sq, sa, n);
    }
    // col[x]: one atomic per wave and row
    const nf_u64 across = nf_wave_sum((nf_u64)q[1] + (nf_u64)q[2] + (nf_u64)q[3]);
    if (lane == 0 && across && x < lx - 1) atomicAdd(&J.col[x], across);
    // the mass: runs of one label along the lanes, summed towards their first lane (k_po_table's scheme): after the step of d a
    // lane holds what the lanes up to 2d - 1 further on in its run have
    if (__ballot(fluid)) {
      const int key = cur.lab;
      const int before = __shfl_up(key, 1);
      const bool head = lane == 0 || before != key;
      const nf_u64 heads = __ballot(head);
      const int run = __popcll(heads & ((2ull << lane) - 1ull));
      nf_u64 massu = (nf_u64)mass;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o_run = __shfl_down(run, d);
        const nf_u64 om = __shfl_down(massu, d);
        if (lane + d < 64 && o_run == run) massu += om;
      }
      if (head && key >= 0 && massu) {
        const int slot = key & (NF_SLOTS - 1);
        const int held = atomicCAS(&s_lab[slot], -1, key);
        if (held == -1 || held == key) atomicAdd(&s_mass[slot], massu);
        else atomicAdd(&J.mass[key], massu);
      }
    }
    cur = nx;
  }
  // row[y]: what the lane above holds for it comes down first
  const nf_u64 from_above = __shfl_down(row_below, 1);
  if (lane < 63) row_here += from_above;
  if (row_here && y < ly - 1) atomicAdd(&J.row[y], row_here);
  if (lane == 0 && row_below && y >= 1 && y <= ly - 1) atomicAdd(&J.row[y - 1], row_below);   // (no lane below it in this wave)
#pragma unroll
  for (int i = 0; i < NF_PLANE_WORDS; ++i) {
    const nf_u64 v = nf_wave_sum(w[i]);
    if (lane == 0 && v) atomicAdd(&s_w[i], v);
  }
  __syncthreads();
  if (threadIdx.x < NF_SLOTS && s_lab[threadIdx.x] >= 0 && s_mass[threadIdx.x]) atomicAdd(&J.mass[s_lab[threadIdx.x]], s_mass[threadIdx.x]);
  if (threadIdx.x < NF_PLANE_WORDS && s_w[threadIdx.x]) atomicAdd(&J.words[threadIdx.x], s_w[threadIdx.x]);
}

__global__ __launch_bounds__(NF_THREADS) void k_nf_tables(const NfJob J) {
  const long t = (long)blockIdx.x * NF_THREADS + threadIdx.x;
  bool flowing = false;
  nf_u64 a = 0;
  if (t < J.L) {
    const lbmdem_net_link e = J.links[t];
    const long long fx = J.out[t].flux_q32;
    a = nf_abs(fx);
    flowing = fx != 0;
    if (flowing && e.lo >= 0 && e.lo < J.B && e.hi >= 0 && e.hi < J.B) {   // (always inside)
      atomicAdd(&J.net[e.hi], (nf_u64)fx);
      atomicAdd(&J.net[e.lo], 0ull - (nf_u64)fx);
      atomicAdd(&J.through[e.lo], a);
      atomicAdd(&J.through[e.hi], a);
    }
  }
  const nf_u64 nflow = __popcll(__ballot(flowing));
  for (int m = 32; m >= 1; m >>= 1) { const nf_u64 o = __shfl_xor(a, m); a = o > a ? o : a; }
  if ((threadIdx.x & 63) == 0) {
    if (nflow) atomicAdd(&J.words[NF_W_FLOWING], nflow);
    if (a) atomicMax(&J.words[NF_W_TOP], a);
  }
}

__global__ __launch_bounds__(NF_THREADS) void k_nf_regions(const NfJob J) {
  const long i = (long)blockIdx.x * NF_THREADS + threadIdx.x;
  const nf_u64 top = J.words[NF_W_TOP];   // (k_nf_tables has finished)
  nf_u64 mine = ~0ull, imb = 0;
  if (i < J.L && nf_abs(J.out[i].flux_q32) == top) mine = (nf_u64)i;
  if (i < J.R) {
    long b = J.level ? (long)J.groups[i].body : i;
    lbmdem_netflux_region r{0, 0, 0};
    if (b >= 0 && b < J.B) {   // (always)
      r.mass_q32 = (long)J.mass[b];
      r.net_q32 = (long)J.net[b];
      r.through_q32 = (long)J.through[b];
    }
    J.regions[i] = r;
    imb = nf_abs(r.net_q32);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const nf_u64 o = __shfl_xor(mine, m), u = __shfl_xor(imb, m);
    mine = o < mine ? o : mine;
    imb = u > imb ? u : imb;
  }
  if ((threadIdx.x & 63) == 0) {
    if (mine != ~0ull) atomicMin(&J.words[NF_W_TOP_LINK], mine);
    if (imb) atomicMax(&J.words[NF_W_IMBALANCE], imb);
  }
}

// what depends on the lattice, once
int netflux_stage(lbmdem_handle* h) {
  auto& V = h->nfx;
  if (V.words) return LBMDEM_OK;
  HIP_TRY(h->mem.dev(&V.col, (size_t)h->L.lx));
  HIP_TRY(h->mem.dev(&V.row, (size_t)h->L.ly));
  HIP_TRY(h->mem.dev(&V.words, (size_t)NF_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

// the pores' guard, and that the network result is the one this result was made over
int netflux_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  const auto& V = h->nfx;
  const auto& W = h->net;
  if (!V.at.current(h) || !W.at.valid || W.gen != V.gen)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_netflux_compute has been made for the map and populations as they are now", who);
  return LBMDEM_OK;
}

int netflux_params(const char* who, int merge, int level) {
  if (level != 0 && level != 1) return fail(LBMDEM_EINVAL, "%s: level must be 0 (between bodies) or 1 (between groups) (%d)", who, level);
  if (merge < -1) return fail(LBMDEM_EINVAL, "%s: merge must be -1 (no merging) or a difference of radii >= 0 (%d)", who, merge);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_netflux_files(const char* dir, int nfile, int lx, int ly, int n, int merge, int level, const lbmdem_net_link* links,
                               const lbmdem_netflux_link* flux, long nlinks, const int* region_body, const long* region_nodes,
                               const lbmdem_netflux_region* regions, long nregions, const long* col, const long* row,
                               const long* counts10, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || merge < -1 || (level != 0 && level != 1) || nlinks < 0 || nregions < 0 || (nlinks > 0 && (!links || !flux)) ||
      (nregions > 0 && (!region_body || !region_nodes || !regions)) || !col || !row || !counts10)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_netflux_files arguments");
  if (lx < 2 || ly < 2 || lx > NF_SIDE_MAX || ly > NF_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_netflux_files: the lattice is %d x %d", lx, ly);
  for (long k = 0; k < nregions; ++k) {
    if (region_body[k] < 0 || (k > 0 && region_body[k] <= region_body[k - 1]))
      return fail(LBMDEM_EINVAL, "lbmdem_write_netflux_files: region %ld has the body %d: the bodies ascend from 0", k, region_body[k]);
    if (region_nodes[k] < 0)
      return fail(LBMDEM_EINVAL, "lbmdem_write_netflux_files: region %ld has %ld nodes: a count is not negative", k, region_nodes[k]);
  }
  for (long k = 0; k < nlinks; ++k) {
    const lbmdem_net_link& e = links[k];
    const bool ascends = k == 0 || e.lo > links[k - 1].lo || (e.lo == links[k - 1].lo && e.hi > links[k - 1].hi);
    if (e.lo < 0 || e.lo >= e.hi || !ascends)
      return fail(LBMDEM_EINVAL, "lbmdem_write_netflux_files: link %ld has the pair (%d, %d): the pairs ascend, 0 <= lo < hi", k, e.lo, e.hi);
    if (flux[k].edges != (long)e.edges)
      return fail(LBMDEM_EINVAL, "lbmdem_write_netflux_files: link %ld has %d edges in the network and %ld in the fluxes", k, e.edges,
                  flux[k].edges);
  }
  OutFile F;
  RC_TRY(F.open("w", dir, "netflux_links%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d level %d\n", lx, ly, n, merge, level);
  fprintf(fp, "# lo hi edges saddle flux_q32 exchange_q32\n");
  for (long k = 0; k < nlinks; ++k)
    fprintf(fp, "%d %d %ld %d %ld %ld\n", links[k].lo, links[k].hi, flux[k].edges, links[k].saddle, flux[k].flux_q32, flux[k].exchange_q32);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "netflux_regions%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d level %d\n", lx, ly, n, merge, level);
  fprintf(fp, "# region body nodes mass_q32 net_q32 through_q32\n");
  for (long k = 0; k < nregions; ++k)
    fprintf(fp, "%ld %d %ld %ld %ld %ld\n", k, region_body[k], region_nodes[k], regions[k].mass_q32, regions[k].net_q32,
            regions[k].through_q32);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "netflux_profile%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d level %d\n", lx, ly, n, merge, level);
  fprintf(fp, "# axis index flux_q32\n");
  for (int x = 0; x < lx - 1; ++x) fprintf(fp, "x %d %ld\n", x, col[x]);
  for (int y = 0; y < ly - 1; ++y) fprintf(fp, "y %d %ld\n", y, row[y]);
  RC_TRY(F.close());
  return stage_append_row(F, dir, "netflux.data",
                          "# t fluid_nodes regions links edges ridge_edges unaccumulated_edges unaccumulated_nodes flowing_links "
                          "strongest_link largest_imbalance", t, counts10, LBMDEM_NETFLUX_COUNTS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_netflux_compute(lbmdem_handle* h, const int*, int, int, long*) { SP_REFUSE(h, "the pore flux analysis"); }
int lbmdem_download_netflux_links(lbmdem_handle* h, lbmdem_netflux_link*, long, long*) { SP_REFUSE(h, "the pore flux analysis"); }
int lbmdem_download_netflux_regions(lbmdem_handle* h, lbmdem_netflux_region*, long, long*) { SP_REFUSE(h, "the pore flux analysis"); }
int lbmdem_download_netflux_profile(lbmdem_handle* h, long*, long*) { SP_REFUSE(h, "the pore flux analysis"); }
int lbmdem_write_netflux(lbmdem_handle* h, const char*, int, int, int) { SP_REFUSE(h, "the pore flux analysis"); }
int lbmdem_set_netflux_output(lbmdem_handle* h, int, int, int) { SP_REFUSE(h, "the pore flux analysis"); }
#else

int lbmdem_netflux_compute(lbmdem_handle* h, const int* map, int merge, int level, long* counts10) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_netflux_compute"));
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  auto& V = h->nfx;
  V.at.valid = false;
  if (lx > NF_SIDE_MAX || ly > NF_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_netflux_compute: a lattice of %d x %d nodes has a side above %d: the squared distances of the "
                               "network underneath are 32-bit integers", lx, ly, NF_SIDE_MAX);
  RC_TRY(netflux_params("lbmdem_netflux_compute", merge, level));
  RC_TRY(stage_check_map("lbmdem_netflux_compute", map, lx, ly, n));
  // the network first: the result of the handle's map is reused while its guard calls it valid and it was made with this merge
  const auto& W = h->net;
  if (map || !(W.at.current(h) && W.own && W.merge == merge)) {
    long nc[LBMDEM_NETWORK_COUNTS];
    RC_TRY(lbmdem_network_compute(h, map, merge, 0, nc));
  }
  RC_TRY(netflux_stage(h));
  const hipStream_t st = h->stream;
  const long B = W.nbodies, nl = W.nlinks[level], R = level ? W.ngroups : W.nbodies;
  HIP_TRY(h->mem.grow(&V.first, &V.first_cap, B + B / 4 + 64));         // (B + 1 are used)
  HIP_TRY(h->mem.grow(&V.sums, &V.sums_cap, 3 * (B + B / 4 + 64)));
  HIP_TRY(h->mem.grow(&V.links, &V.link_cap, nl + nl / 4 + 64));
  HIP_TRY(h->mem.grow(&V.regions, &V.region_cap, R + R / 4 + 64));
  NfJob J{};
  J.f = h->f[h->fcur];
  J.lab = level ? W.group : W.body;
  J.lx = lx; J.ly = ly; J.sy = sy;
  J.B = B;
  J.links = W.links[level]; J.L = nl;
  J.first = V.first;
  J.mass = V.sums; J.net = V.sums + (B > 0 ? B : 1); J.through = V.sums + 2 * (B > 0 ? B : 1);
  J.out = V.links;
  J.col = reinterpret_cast<nf_u64*>(V.col); J.row = reinterpret_cast<nf_u64*>(V.row);
  J.words = V.words;
  J.groups = W.groups; J.R = R; J.level = level;
  J.regions = V.regions;
  HIP_TRY(hipMemsetAsync(V.words, 0, sizeof(nf_u64) * NF_WORDS, st));
  HIP_TRY(hipMemsetAsync(V.words + NF_W_TOP_LINK, 0xFF, sizeof(nf_u64), st));   // (a minimum)
  HIP_TRY(hipMemsetAsync(V.col, 0, sizeof(long) * (size_t)lx, st));
  HIP_TRY(hipMemsetAsync(V.row, 0, sizeof(long) * (size_t)ly, st));
  HIP_TRY(hipMemsetAsync(V.sums, 0, sizeof(nf_u64) * 3 * (size_t)(B > 0 ? B : 1), st));
  HIP_TRY(hipMemsetAsync(V.links, 0, sizeof(lbmdem_netflux_link) * (size_t)(nl > 0 ? nl : 1), st));
  hipLaunchKernelGGL(k_nf_first, dim3((unsigned)stage_blocks(B + 1, NF_THREADS)), dim3(NF_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nf_plane, dim3((unsigned)stage_blocks(sy, NF_THREADS), (unsigned)stage_blocks(lx, NF_ROWS)), dim3(NF_THREADS), 0, st, J);
  if (nl > 0) hipLaunchKernelGGL(k_nf_tables, dim3((unsigned)stage_blocks(nl, NF_THREADS)), dim3(NF_THREADS), 0, st, J);
  const long items = nl > R ? nl : R;
  if (items > 0) hipLaunchKernelGGL(k_nf_regions, dim3((unsigned)stage_blocks(items, NF_THREADS)), dim3(NF_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[NF_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts10[0] = (long)w[NF_W_FLUID];
  counts10[1] = R;
  counts10[2] = nl;
  counts10[3] = (long)w[NF_W_EDGES];
  counts10[4] = (long)w[NF_W_RIDGE];
  counts10[5] = (long)w[NF_W_BAD_EDGES];
  counts10[6] = (long)w[NF_W_BAD_NODES];
  counts10[7] = (long)w[NF_W_FLOWING];
  counts10[8] = nl > 0 ? (long)w[NF_W_TOP_LINK] : -1;
  counts10[9] = (long)w[NF_W_IMBALANCE];
  V.nlinks = nl; V.nregions = R;
  V.merge = merge; V.level = level;
  V.gen = W.gen;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_netflux_links(lbmdem_handle* h, lbmdem_netflux_link* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(netflux_ready(h, "lbmdem_download_netflux_links"));
  return stage_table(h, "lbmdem_download_netflux_links", "links", h->nfx.links, sizeof *out, h->nfx.nlinks, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_netflux_regions(lbmdem_handle* h, lbmdem_netflux_region* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(netflux_ready(h, "lbmdem_download_netflux_regions"));
  return stage_table(h, "lbmdem_download_netflux_regions", "regions", h->nfx.regions, sizeof *out, h->nfx.nregions, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_netflux_profile(lbmdem_handle* h, long* col, long* row) try {
  CHECK_H(h);
  if (!col && !row) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(netflux_ready(h, "lbmdem_download_netflux_profile"));
  const LatticeView& L = h->L;
  if (col && L.lx > 1) HIP_TRY(hipMemcpyAsync(col, h->nfx.col, sizeof(long) * (size_t)(L.lx - 1), hipMemcpyDeviceToHost, h->stream));
  if (row && L.ly > 1) HIP_TRY(hipMemcpyAsync(row, h->nfx.row, sizeof(long) * (size_t)(L.ly - 1), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_netflux(lbmdem_handle* h, const char* dir, int nfile, int merge, int level) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_netflux"));
  const LatticeView& L = h->L;
  long counts[LBMDEM_NETFLUX_COUNTS], nl = 0, nf = 0, nr = 0, nb = 0, ng = 0;
  RC_TRY(lbmdem_netflux_compute(h, nullptr, merge, level, counts));
  RC_TRY(lbmdem_download_network_links(h, level, nullptr, 0, &nl));
  RC_TRY(lbmdem_download_netflux_links(h, nullptr, 0, &nf));
  RC_TRY(lbmdem_download_netflux_regions(h, nullptr, 0, &nr));
  std::vector<lbmdem_net_link> links((size_t)nl);
  std::vector<lbmdem_netflux_link> flux((size_t)nf);
  std::vector<lbmdem_netflux_region> regions((size_t)nr);
  std::vector<int> body((size_t)nr);
  std::vector<long> nodes((size_t)nr), col((size_t)L.lx), row((size_t)L.ly);
  if (nl > 0) RC_TRY(lbmdem_download_network_links(h, level, links.data(), nl, &nl));
  if (nf > 0) RC_TRY(lbmdem_download_netflux_links(h, flux.data(), nf, &nf));
  if (nr > 0) RC_TRY(lbmdem_download_netflux_regions(h, regions.data(), nr, &nr));
  if (level == 0) {
    RC_TRY(lbmdem_download_network_bodies(h, nullptr, 0, &nb));
    std::vector<lbmdem_net_body> bodies((size_t)nb);
    if (nb > 0) RC_TRY(lbmdem_download_network_bodies(h, bodies.data(), nb, &nb));
    for (long k = 0; k < nr && k < nb; ++k) { body[(size_t)k] = (int)k; nodes[(size_t)k] = bodies[(size_t)k].nodes; }
  } else {
    RC_TRY(lbmdem_download_network_groups(h, nullptr, 0, &ng));
    std::vector<lbmdem_net_group> groups((size_t)ng);
    if (ng > 0) RC_TRY(lbmdem_download_network_groups(h, groups.data(), ng, &ng));
    for (long k = 0; k < nr && k < ng; ++k) { body[(size_t)k] = groups[(size_t)k].body; nodes[(size_t)k] = groups[(size_t)k].nodes; }
  }
  RC_TRY(lbmdem_download_netflux_profile(h, col.data(), row.data()));
  return lbmdem_write_netflux_files(dir, nfile, L.lx, L.ly, h->n, merge, level, nl > 0 ? links.data() : nullptr,
                                    nf > 0 ? flux.data() : nullptr, nl, nr > 0 ? body.data() : nullptr, nr > 0 ? nodes.data() : nullptr,
                                    nr > 0 ? regions.data() : nullptr, nr, col.data(), row.data(), counts, h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_netflux_output(lbmdem_handle* h, int on, int merge, int level) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_netflux_output"));
    RC_TRY(netflux_params("lbmdem_set_netflux_output", merge, level));
    h->netflux_merge = merge;
    h->netflux_level = level;
  }
  h->netflux_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
