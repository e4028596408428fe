// lbm_geodesic.hip -- geodesic distance through the pore space: for every passable fluid node the length of the shortest path of
// adjacent passable nodes from an inlet region (dist), on request the same from an outlet region (back) and from the two the
// corridor of shortest paths between them (detour == 0), a profile over the depth behind the inlet and ten counts
// (lbmdem_geodesic_compute, lbmdem_download_geodesic, lbmdem_geodesic_device, lbmdem_download_geodesic_profile,
// lbmdem_geodesic_rounds, lbmdem_write_geodesic, lbmdem_set_geodesic_output, lbmdem_write_geodesic_files; include/lbmdem_hip.h,
// "Geodesic", has the contract in full). Every result is an integer: an axis step costs 5, a diagonal one 7. The distances are the
// greatest fixed point below the seed of D[p] = min(D[p], D[q] + w(p, q)): values only fall, and only to values a real path
// realises, so any order of relaxations ends at the same plane. Nothing here is on the step path: the kernels read the map (or the
// ClearanceStage's d2 when min_d2 > 1) and write to the handle's GeodesicStage; nothing is allocated or launched before the first
// compute.
//
// In the device layout (node = x*sy + y), on the handle's stream:
//   k_geo_seed     lanes along y, GEO_ROWS rows per workgroup: 0 on the passable nodes of the region, INT_MAX on the other passable
//                  nodes, -1 elsewhere (the pad columns too); the counts of fluid, passable and region nodes (a wavefront's lanes
//                  summed first, then LDS, then 64-bit atomics); the tiles that hold a seed go on the first list;
//   k_geo_relax    in rounds over the list of active tiles, one workgroup per tile of 16 x 64 nodes, y along the lanes: the tile and
//                  an apron of one node into LDS (relaxed agent-scope loads: a stale value is only a larger one), sweeps in LDS
//                  until one lowers nothing, GEO_SWEEPS at most, then the lowered nodes of its own interior back to memory. A tile
//                  puts on the next round's list each of its 8 neighbours that shares a border node it lowered (in the first round
//                  also a border node that is a seed: nobody has looked at it yet), and itself if it stopped at the bound. A tile is on a list once: its stamp says which round it was last listed for. The host reads
//                  the next list's length after every launch and stops at the first launch that lists nothing. No workgroup waits
//                  for another; every loop has the bound its comment states;
//   k_geo_finish   lanes along y: INT_MAX -> -1, the reached nodes, the largest distance, over the outlet the minimum of
//                  dist << 32 | k: shortest and shortest_node, and the profile (per lane a run of equal depth in registers, per
//                  workgroup LDS bins, then 64-bit atomics; least and largest by atomic min / max);
//   k_geo_detour   one lane per node: detour (shortest is there by now) and path_nodes.
// Integer atomics only, no floating point in a kernel.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both. Front end, as every export's: whole_handle(), SP_REFUSE() (lbmdem_handle.h), MemPool (lbm_mem.h), OutFile (lbm_outfile.h),
// lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>

namespace {

constexpr int GEO_SIDE_MAX = 32768;   // the clearance analysis'

#ifndef LBMDEM_SINGLE_PRECISION
typedef unsigned long long geo_u64;
constexpr int GEO_THREADS = 256;
constexpr int GEO_ROWS = 32;          // rows per workgroup of the seed and finish passes
constexpr int GEO_TX = 16, GEO_TY = 64;   // a tile of the relaxation: 16 rows of 64 nodes, y along the lanes
constexpr int GEO_PER = GEO_TX / (GEO_THREADS / 64);   // rows of a tile per lane: 4
constexpr int GEO_PITCH = GEO_TY + 2;
constexpr int GEO_SWEEPS = 128;       // sweeps per workgroup and launch at most
constexpr int GEO_INF = INT_MAX;      // passable, not reached (in LDS: not passable too)
constexpr int GEO_FBINS = GEO_THREADS, GEO_GBINS = GEO_ROWS;   // the depths a workgroup of the finish pass can meet: along y, along x
constexpr int GEO_BINS = GEO_FBINS + GEO_GBINS;
// GeodesicStage::words
enum : int { GEO_W_FLUID = 0, GEO_W_PASSABLE, GEO_W_INLET, GEO_W_BACK0, GEO_W_BACK1, GEO_W_BACK2, GEO_W_REACHED, GEO_W_OUTLET,
             GEO_W_OUTLET_REACHED, GEO_W_PATH, GEO_W_MAX, GEO_W_SHORTEST, GEO_WORDS };

struct GeoJob {
  const int* M;      // [lx][sy] the map (min_d2 <= 1), or null
  const int* d2;     // [lx][sy] the clearance analysis' plane (min_d2 > 1), or null
  int min_d2;
  int lx, ly, sy, conn, band, from, to;
  long N;            // lx * sy
  int ntx, nty;      // tiles along x and y
  int* plane;        // the plane this pass seeds and relaxes: dist or back
  int mask;          // ... from the region of this mask
  int wbase;         // ... with the seed's three counts at words + wbase
  int* dist;
  int* back;
  int* detour;
  int* stamp;        // [ntx * nty] the round a tile was last listed for
  const int* list_in;
  int* list_out;
  unsigned* cnt_out; // the length of list_out
  int next;          // the stamp of the round list_out is for
  geo_u64* words;
  geo_u64* lev;      // [3][nd] per depth: passable nodes, reached ones, the sum of their dist
  int* lmin;         // [nd] the least dist (above INT_MAX / 2 without one)
  int* lmax;         // [nd] the largest, -1 without one
  int nd;
};

__device__ __forceinline__ int geo_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void geo_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned geo_lds(const int* p) { return (unsigned)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the region of a side mask: B 1 (y low), T 2 (y high), L 4 (x low), R 8 (x high), `band` nodes deep (drainage's)
__device__ __forceinline__ bool geo_region(const GeoJob& J, int mask, int x, int y) {
  return ((mask & 1) && y < J.band) || ((mask & 2) && y >= J.ly - J.band) || ((mask & 4) && x < J.band) || ((mask & 8) && x >= J.lx - J.band);
}

// a tile goes on the next round's list, once
__device__ __forceinline__ void geo_list(const GeoJob& J, int t) {
  if (__hip_atomic_exchange(J.stamp + t, J.next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == J.next) return;
  const unsigned k = atomicAdd(J.cnt_out, 1u);
  if (k < (unsigned)(J.ntx * J.nty)) J.list_out[k] = t;   // (always: a tile is listed once a round)
}

__device__ __forceinline__ geo_u64 geo_wave_sum(geo_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}
__device__ __forceinline__ geo_u64 geo_wave_max(geo_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) { const geo_u64 o = __shfl_xor(v, m); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ geo_u64 geo_wave_min(geo_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) { const geo_u64 o = __shfl_xor(v, m); v = o < v ? o : v; }
  return v;
}

__global__ __launch_bounds__(GEO_THREADS) void k_geo_seed(const GeoJob J) {
  __shared__ geo_u64 s_w[3];
  if (threadIdx.x < 3) s_w[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * GEO_THREADS + threadIdx.x;   // (a wavefront lies in one column of tiles: 256 and 64 divide)
  const int lx = J.lx, ly = J.ly, sy = J.sy;
  geo_u64 w[3] = {};
  bool seen = false;   // a seed in this lane since the last row of tiles began
  for (int r = 0; r < GEO_ROWS; ++r) {
    const int x = blockIdx.y * GEO_ROWS + r;
    if (x >= lx) break;   // (the whole workgroup)
    const long node = (long)x * sy + y;
    bool fluid = false, pass = false;
    if (y < ly) {
      if (J.d2) { const int d = J.d2[node]; fluid = d > 0; pass = fluid && d >= J.min_d2; }
      else fluid = pass = J.M[node] == -1;
    }
    const bool seed = pass && geo_region(J, J.mask, x, y);
    if (y < sy) J.plane[node] = pass ? (seed ? 0 : GEO_INF) : -1;   // (the pad columns: -1)
    w[0] += fluid; w[1] += pass; w[2] += seed;
    seen = seen || seed;
    if ((x % GEO_TX) == GEO_TX - 1 || x == lx - 1 || r == GEO_ROWS - 1) {
      if (__any(seen) && lane == 0) geo_list(J, (x / GEO_TX) * J.nty + y / GEO_TY);   // (lane 0's y is inside: y0 < sy rounded down)
      seen = false;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const geo_u64 v = geo_wave_sum(w[i]);
    if (lane == 0 && v) atomicAdd(&s_w[i], v);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_w[threadIdx.x]) atomicAdd(&J.words[J.wbase + threadIdx.x], s_w[threadIdx.x]);
}

__global__ __launch_bounds__(GEO_THREADS) void k_geo_relax(const GeoJob J) {
  __shared__ int s[GEO_TX + 2][GEO_PITCH];
  __shared__ int s_mark;
  const int t = J.list_in[blockIdx.x];
  if (t < 0 || t >= J.ntx * J.nty) return;   // (never; the whole workgroup)
  const int tx = t / J.nty, ty = t % J.nty;
  const int x0 = tx * GEO_TX, y0 = ty * GEO_TY;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lx = J.lx, ly = J.ly, sy = J.sy;
  if (tid == 0) s_mark = 0;
  int cur[GEO_PER], orig[GEO_PER];
#pragma unroll
  for (int k = 0; k < GEO_PER; ++k) {
    const int x = x0 + wv * GEO_PER + k, y = y0 + lane;
    int v = -1;
    if (x < lx && y < ly) v = geo_load(J.plane + (long)x * sy + y);
    orig[k] = cur[k] = v;   // (>= 0 exactly on the passable nodes)
    s[1 + wv * GEO_PER + k][1 + lane] = v < 0 ? GEO_INF : v;
  }
  if (tid < 2 * GEO_PITCH + 2 * GEO_TX) {   // the apron: two rows of 66, two columns of 16
    int r, c;
    if (tid < GEO_PITCH) { r = 0; c = tid; }
    else if (tid < 2 * GEO_PITCH) { r = GEO_TX + 1; c = tid - GEO_PITCH; }
    else if (tid < 2 * GEO_PITCH + GEO_TX) { r = 1 + tid - 2 * GEO_PITCH; c = 0; }
    else { r = 1 + tid - 2 * GEO_PITCH - GEO_TX; c = GEO_TY + 1; }
    const int x = x0 - 1 + r, y = y0 - 1 + c;
    int v = -1;
    if (x >= 0 && x < lx && y >= 0 && y < ly) v = geo_load(J.plane + (long)x * sy + y);
    s[r][c] = v < 0 ? GEO_INF : v;
  }
  __syncthreads();
  const bool diag = J.conn == 8;
  int busy = 0;
  // a sweep: every lane its rows down and up again, reading whatever its neighbours hold by now. A node is written by its own lane
  // only, and only lowered to a neighbour's value plus the step: a quiet sweep read the final state. GEO_SWEEPS sweeps at most.
  for (int sweep = 0; sweep < GEO_SWEEPS; ++sweep) {
    int ch = 0;
#pragma unroll
    for (int kk = 0; kk < 2 * GEO_PER; ++kk) {
      const int k = kk < GEO_PER ? kk : 2 * GEO_PER - 1 - kk;
      if (orig[k] < 0) continue;
      const int r = 1 + wv * GEO_PER + k, c = 1 + lane;
      unsigned a = geo_lds(&s[r - 1][c]), b = geo_lds(&s[r + 1][c]);
      a = a < b ? a : b;
      b = geo_lds(&s[r][c - 1]); a = a < b ? a : b;
      b = geo_lds(&s[r][c + 1]); a = a < b ? a : b;
      a += 5u;   // (INT_MAX + 7 does not wrap an unsigned)
      if (diag) {
        unsigned d = geo_lds(&s[r - 1][c - 1]);
        b = geo_lds(&s[r - 1][c + 1]); d = d < b ? d : b;
        b = geo_lds(&s[r + 1][c - 1]); d = d < b ? d : b;
        b = geo_lds(&s[r + 1][c + 1]); d = d < b ? d : b;
        d += 7u;
        a = a < d ? a : d;
      }
      if (a < (unsigned)cur[k]) {
        cur[k] = (int)a;
        __hip_atomic_store(&s[r][c], (int)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ch = 1;
      }
    }
    busy = __syncthreads_or(ch);   // (the same in every lane)
    if (!busy) break;
  }
  // the lowered nodes back to memory, and who has to look again: bit 3 * (dx + 1) + (dy + 1), bit 4 is the tile itself
  // (in the first round a seed on the border counts as lowered: the tile next to it has not seen it yet)
  int mk = 0;
  const bool first = J.next == 2;
#pragma unroll
  for (int k = 0; k < GEO_PER; ++k) {
    if (cur[k] >= orig[k] && !(first && orig[k] == 0)) continue;
    const int r = wv * GEO_PER + k;
    if (cur[k] < orig[k]) geo_store(J.plane + (long)(x0 + r) * sy + y0 + lane, cur[k]);   // (a passable node: inside the lattice)
    const int dx = r == 0 ? -1 : r == GEO_TX - 1 ? 1 : 0, dy = lane == 0 ? -1 : lane == GEO_TY - 1 ? 1 : 0;
    if (dx) mk |= 1 << (3 * (dx + 1) + 1);
    if (dy) mk |= 1 << (3 + dy + 1);
    if (dx && dy) mk |= 1 << (3 * (dx + 1) + dy + 1);
  }
  if (busy && tid == 0) mk |= 1 << 4;
  if (mk) atomicOr(&s_mark, mk);
  __syncthreads();
  if (tid < 9 && (s_mark >> tid & 1)) {
    const int nx = tx + tid / 3 - 1, ny = ty + tid % 3 - 1;
    if (nx >= 0 && nx < J.ntx && ny >= 0 && ny < J.nty) geo_list(J, nx * J.nty + ny);
  }
}

// depth(p): the least offset to a side in `from`; along y (B, T) and along x (L, R), INT_MAX where the mask has neither
__device__ __forceinline__ int geo_depth_y(const GeoJob& J, int y) {
  int d = INT_MAX;
  if (J.from & 1) d = y;
  if ((J.from & 2) && J.ly - 1 - y < d) d = J.ly - 1 - y;
  return d;
}
__device__ __forceinline__ int geo_depth_x(const GeoJob& J, int x) {
  int d = INT_MAX;
  if (J.from & 4) d = x;
  if ((J.from & 8) && J.lx - 1 - x < d) d = J.lx - 1 - x;
  return d;
}

struct GeoRun {   // a lane's nodes of one depth in a row
  int bin, dmin, dmax;
  unsigned nodes, reached;
  geo_u64 sum;
};

__global__ __launch_bounds__(GEO_THREADS) void k_geo_finish(const GeoJob J) {
  __shared__ unsigned s_nodes[GEO_BINS], s_reached[GEO_BINS];
  __shared__ geo_u64 s_sum[GEO_BINS];
  __shared__ int s_min[GEO_BINS], s_max[GEO_BINS];
  __shared__ int s_f0, s_g0;   // the least depth along y and along x this workgroup meets: bin 0 of either part
  __shared__ geo_u64 s_w[GEO_WORDS];
  for (int i = threadIdx.x; i < GEO_BINS; i += GEO_THREADS) { s_nodes[i] = s_reached[i] = 0; s_sum[i] = 0; s_min[i] = INT_MAX; s_max[i] = -1; }
  if (threadIdx.x < GEO_WORDS) s_w[threadIdx.x] = threadIdx.x == GEO_W_SHORTEST ? ~0ull : 0ull;
  if (threadIdx.x == 0) { s_f0 = INT_MAX; s_g0 = INT_MAX; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * GEO_THREADS + threadIdx.x;
  const int lx = J.lx, ly = J.ly, sy = J.sy;
  const int fy = y < ly ? geo_depth_y(J, y) : INT_MAX;
  if (fy != INT_MAX) atomicMin(&s_f0, fy);
  if (threadIdx.x < GEO_ROWS && blockIdx.y * GEO_ROWS + (int)threadIdx.x < lx) {
    const int gx = geo_depth_x(J, blockIdx.y * GEO_ROWS + threadIdx.x);
    if (gx != INT_MAX) atomicMin(&s_g0, gx);
  }
  __syncthreads();
  const int f0 = s_f0, g0 = s_g0;
  geo_u64 reached = 0, outlet = 0, outlet_reached = 0, top = 0, shortest = ~0ull;
  GeoRun R{-1, INT_MAX, -1, 0, 0, 0};
  auto flush = [&]() {   // (depths along y span < 256 values in a workgroup, along x < 32: the bin is inside)
    if (R.bin >= 0 && R.bin < GEO_BINS && R.nodes) {
      atomicAdd(&s_nodes[R.bin], R.nodes);
      if (R.reached) {
        atomicAdd(&s_reached[R.bin], R.reached);
        atomicAdd(&s_sum[R.bin], R.sum);
        atomicMin(&s_min[R.bin], R.dmin);
        atomicMax(&s_max[R.bin], R.dmax);
      }
    }
    R = GeoRun{-1, INT_MAX, -1, 0, 0, 0};
  };
  for (int r = 0; r < GEO_ROWS; ++r) {
    const int x = blockIdx.y * GEO_ROWS + r;
    if (x >= lx) break;   // (the whole workgroup)
    if (y >= ly) continue;   // (the pad columns hold -1 since the seed)
    const long node = (long)x * sy + y;
    int d = J.dist[node];
    if (d < 0) continue;   // not passable
    if (d == GEO_INF) { d = -1; J.dist[node] = -1; }
    if (J.to) {
      const int b = J.back[node];
      if (b == GEO_INF) J.back[node] = -1;
    }
    const int gx = geo_depth_x(J, x);
    const int bin = fy <= gx ? fy - f0 : GEO_FBINS + gx - g0;
    if (bin != R.bin) { flush(); R.bin = bin; }
    R.nodes += 1;
    if (d >= 0) {
      R.reached += 1; R.sum += (geo_u64)d;
      R.dmin = d < R.dmin ? d : R.dmin; R.dmax = d > R.dmax ? d : R.dmax;
      reached += 1;
      if ((geo_u64)d + 1 > top) top = (geo_u64)d + 1;
    }
    if (J.to && geo_region(J, J.to, x, y)) {
      outlet += 1;
      if (d >= 0) {
        outlet_reached += 1;
        const geo_u64 mine = (geo_u64)(unsigned)d << 32 | (geo_u64)(unsigned)((long)x * ly + y);   // the smaller index wins
        shortest = mine < shortest ? mine : shortest;
      }
    }
  }
  flush();
  geo_u64 v;
  v = geo_wave_sum(reached); if (lane == 0 && v) atomicAdd(&s_w[GEO_W_REACHED], v);
  v = geo_wave_sum(outlet); if (lane == 0 && v) atomicAdd(&s_w[GEO_W_OUTLET], v);
  v = geo_wave_sum(outlet_reached); if (lane == 0 && v) atomicAdd(&s_w[GEO_W_OUTLET_REACHED], v);
  v = geo_wave_max(top); if (lane == 0 && v) atomicMax(&s_w[GEO_W_MAX], v);
  v = geo_wave_min(shortest); if (lane == 0 && v != ~0ull) atomicMin(&s_w[GEO_W_SHORTEST], v);
  __syncthreads();
  for (int i = threadIdx.x; i < GEO_BINS; i += GEO_THREADS) {
    if (!s_nodes[i]) continue;
    const long dep = i < GEO_FBINS ? (long)f0 + i : (long)g0 + i - GEO_FBINS;
    if (dep < 0 || dep >= J.nd) continue;   // (never)
    atomicAdd(&J.lev[dep], (geo_u64)s_nodes[i]);
    if (s_reached[i]) {
      atomicAdd(&J.lev[J.nd + dep], (geo_u64)s_reached[i]);
      atomicAdd(&J.lev[2 * (long)J.nd + dep], s_sum[i]);
      atomicMin(&J.lmin[dep], s_min[i]);
      atomicMax(&J.lmax[dep], s_max[i]);
    }
  }
  if (threadIdx.x == GEO_W_REACHED || threadIdx.x == GEO_W_OUTLET || threadIdx.x == GEO_W_OUTLET_REACHED) {
    if (s_w[threadIdx.x]) atomicAdd(&J.words[threadIdx.x], s_w[threadIdx.x]);
  } else if (threadIdx.x == GEO_W_MAX) {
    if (s_w[threadIdx.x]) atomicMax(&J.words[threadIdx.x], s_w[threadIdx.x]);
  } else if (threadIdx.x == GEO_W_SHORTEST) {
    if (s_w[threadIdx.x] != ~0ull) atomicMin(&J.words[threadIdx.x], s_w[threadIdx.x]);
  }
}

__global__ __launch_bounds__(GEO_THREADS) void k_geo_detour(const GeoJob J) {
  const long node = (long)blockIdx.x * GEO_THREADS + threadIdx.x;
  const geo_u64 key = J.words[GEO_W_SHORTEST];   // (k_geo_finish has finished)
  bool on_path = false;
  if (node < J.N) {
    int v = -1;
    if (key != ~0ull) {
      const int d = J.dist[node], b = J.back[node];
      if (d >= 0 && b >= 0) {
        const long long dt = (long long)d + b - (long long)(key >> 32);   // (>= 0: a path over this node is no shorter)
        v = dt > INT_MAX ? INT_MAX : (int)dt;
        on_path = v == 0;
      }
    }
    J.detour[node] = v;
  }
  const geo_u64 n = __popcll(__ballot(on_path));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&J.words[GEO_W_PATH], n);
}

// the largest depth on the lattice: depth = min(along y, along x), and the two vary independently
int geo_depthmax(int lx, int ly, int from) {
  int dy = INT_MAX, dx = INT_MAX;
  if (from & 3) dy = (from & 3) == 3 ? (ly - 1) / 2 : ly - 1;
  if (from & 12) dx = (from & 12) == 12 ? (lx - 1) / 2 : lx - 1;
  return dy < dx ? dy : dx;
}

// what depends on the lattice, once
int geodesic_stage(lbmdem_handle* h) {
  auto& V = h->geo;
  if (V.words) return LBMDEM_OK;
  const size_t N = (size_t)h->L.lx * h->L.sy;
  const size_t tiles = (size_t)stage_blocks(h->L.lx, GEO_TX) * (size_t)stage_blocks(h->L.ly, GEO_TY);
  HIP_TRY(h->mem.dev(&V.dist, N));
  HIP_TRY(h->mem.dev(&V.back, N));
  HIP_TRY(h->mem.dev(&V.detour, N));
  HIP_TRY(h->mem.dev(&V.stamp, tiles));
  HIP_TRY(h->mem.dev(&V.list, 2 * tiles));
  HIP_TRY(h->mem.dev(&V.cnt, (size_t)2));
  HIP_TRY(h->mem.dev(&V.words, (size_t)GEO_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

// one relaxation: the seed, then rounds until a launch lists nothing -> *rounds, the launches
int geodesic_pass(lbmdem_handle* h, GeoJob J, int* plane, int mask, int wbase, int* rounds) {
  auto& V = h->geo;
  const hipStream_t st = h->stream;
  const long tiles = (long)J.ntx * J.nty;
  J.plane = plane; J.mask = mask; J.wbase = wbase;
  HIP_TRY(hipMemsetAsync(V.stamp, 0, sizeof(int) * (size_t)tiles, st));
  HIP_TRY(hipMemsetAsync(V.cnt, 0, sizeof(unsigned) * 2, st));
  J.next = 1; J.list_in = nullptr; J.list_out = V.list; J.cnt_out = V.cnt;
  hipLaunchKernelGGL(k_geo_seed, dim3((unsigned)stage_blocks(J.sy, GEO_THREADS), (unsigned)stage_blocks(J.lx, GEO_ROWS)), dim3(GEO_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned listed = 0;
  unsigned long long passable = 0;
  HIP_TRY(hipMemcpyAsync(&listed, V.cnt, sizeof listed, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&passable, V.words + wbase + 1, sizeof passable, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *rounds = 0;
  // a launch that lists something has lowered a node: passable_nodes launches at most do, one more is quiet
  for (long round = 1; listed > 0; ++round) {
    if (round > (long)passable + 2)
      return fail(LBMDEM_EINVAL, "lbmdem_geodesic_compute: the relaxation did not settle in %ld rounds", (long)passable + 2);
    if (listed > (unsigned long long)tiles) return fail(LBMDEM_EINVAL, "lbmdem_geodesic_compute: %u of %ld tiles are listed", listed, tiles);
    const int in = (int)((round - 1) & 1), out = 1 - in;
    J.list_in = V.list + in * tiles; J.list_out = V.list + out * tiles; J.cnt_out = V.cnt + out;
    J.next = (int)(round + 1);   // (round <= lx * ly + 2 < INT_MAX)
    HIP_TRY(hipMemsetAsync(J.cnt_out, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_geo_relax, dim3(listed), dim3(GEO_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&listed, J.cnt_out, sizeof listed, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *rounds = (int)round;
  }
  return LBMDEM_OK;
}

// the pores' guard, and with min_d2 > 1 over the handle's map that the clearance result underneath is still the one
int geodesic_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  const auto& V = h->geo;
  const auto& Q = h->clr;
  if (!V.at.current(h) || (V.over_clearance && (!Q.at.valid || Q.gen != V.gen)))
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_geodesic_compute has been made for the map as it is now", who);
  return LBMDEM_OK;
}

int geodesic_args(const char* who, int from, int band, int to, int conn, int min_d2) {
  RC_TRY(stage_check_sides(who, from, band, to));
  if (conn != 4 && conn != 8) return fail(LBMDEM_EINVAL, "%s: conn must be 4 or 8 (%d)", who, conn);
  if (min_d2 < 0) return fail(LBMDEM_EINVAL, "%s: min_d2 must not be negative (%d)", who, min_d2);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_geodesic_files(const char* dir, int nfile, int lx, int ly, int n, int from, int band, int to, int conn, int min_d2,
                                int plane, const int* dist, const int* back, const int* detour, const lbmdem_geo_level* levels,
                                long nlevels, const long* counts10, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || nlevels < 1 || !levels || !counts10 || (plane && (!dist || !back || !detour)) || from < 1 || from > 15 || to < 0 ||
      to > 15 || band < 1 || (conn != 4 && conn != 8) || min_d2 < 0)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_geodesic_files arguments");
  if (lx < 2 || ly < 2 || lx > GEO_SIDE_MAX || ly > GEO_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_geodesic_files: the lattice is %d x %d", lx, ly);
  for (long k = 0; k < nlevels; ++k) {
    const lbmdem_geo_level& e = levels[k];
    if (e.nodes < 0 || e.reached < 0 || e.reached > e.nodes || e.sum < 0)
      return fail(LBMDEM_EINVAL, "lbmdem_write_geodesic_files: depth %ld has %ld nodes, %ld reached and the sum %ld: 0 <= reached <= nodes, "
                                 "0 <= sum", k, e.nodes, e.reached, e.sum);
    if (e.reached == 0 ? (e.dmin != -1 || e.dmax != -1) : (e.dmin < 0 || e.dmax < e.dmin))
      return fail(LBMDEM_EINVAL, "lbmdem_write_geodesic_files: depth %ld has the least distance %d and the largest %d over %ld reached "
                                 "nodes", k, e.dmin, e.dmax, e.reached);
  }
  const long cnt = (long)lx * ly;
  const int* const planes[3] = {dist, back, detour};
  const char* const names[3] = {"dist", "back", "detour"};
  if (plane)
    for (int i = 0; i < 3; ++i)
      for (long k = 0; k < cnt; ++k)
        if (planes[i][k] < -1)
          return fail(LBMDEM_EINVAL, "lbmdem_write_geodesic_files: %s[%ld][%ld] = %d is below -1", names[i], k / ly, k % ly, planes[i][k]);
  OutFile F;
  RC_TRY(F.open("w", dir, "geodesic_profile%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d from %d band %d to %d conn %d min_d2 %d\n", lx, ly, n, from, band, to, conn, min_d2);
  fprintf(fp, "# depth nodes reached sum min max tortuosity\n");
  for (long k = 0; k < nlevels; ++k) {
    const lbmdem_geo_level& e = levels[k];
    double tau = 0.;
    if (k >= band && e.reached > 0) tau = (double)e.sum / (double)((long)LBMDEM_GEO_UNIT * e.reached * (k - band + 1));
    fprintf(fp, "%ld %ld %ld %ld %d %d %.6f\n", k, e.nodes, e.reached, e.sum, e.dmin, e.dmax, tau);
  }
  RC_TRY(F.close());
  if (plane) RC_TRY(stage_write_int_planes(F, dir, nfile, "geodesic%.6i.vtk", "lbmdem geodesic", lx, ly, names, planes, 3));
  return stage_append_row(F, dir, "geodesic.data",
                          "# t fluid_nodes passable_nodes inlet_nodes reached_nodes dist_max outlet_nodes outlet_reached shortest "
                          "shortest_node path_nodes", t, counts10, LBMDEM_GEODESIC_COUNTS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_geodesic_compute(lbmdem_handle* h, const int*, int, int, int, int, int, long, long*) { SP_REFUSE(h, "the geodesic analysis"); }
int lbmdem_download_geodesic(lbmdem_handle* h, int*, int*, int*) { SP_REFUSE(h, "the geodesic analysis"); }
int lbmdem_geodesic_device(lbmdem_handle* h, const int**, const int**, const int**, int*) { SP_REFUSE(h, "the geodesic analysis"); }
int lbmdem_download_geodesic_profile(lbmdem_handle* h, lbmdem_geo_level*, long, long*) { SP_REFUSE(h, "the geodesic analysis"); }
int lbmdem_geodesic_rounds(lbmdem_handle* h, int*, int*) { SP_REFUSE(h, "the geodesic analysis"); }
int lbmdem_write_geodesic(lbmdem_handle* h, const char*, int, int, int, int, int, int, int) { SP_REFUSE(h, "the geodesic analysis"); }
int lbmdem_set_geodesic_output(lbmdem_handle* h, int, int, int, int, int, int, int) { SP_REFUSE(h, "the geodesic analysis"); }
#else

int lbmdem_geodesic_compute(lbmdem_handle* h, const int* map, int from, int band, int to, int conn, int min_d2, long max_edges,
                            long* counts10) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_geodesic_compute"));
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  auto& V = h->geo;
  V.at.valid = false;
  RC_TRY(geodesic_args("lbmdem_geodesic_compute", from, band, to, conn, min_d2));
  if (lx > GEO_SIDE_MAX || ly > GEO_SIDE_MAX || 7 * (long)lx * ly > (long)INT_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_geodesic_compute: a lattice of %d x %d nodes has a side above %d or more than %d nodes: a "
                               "distance is a 32-bit integer", lx, ly, GEO_SIDE_MAX, INT_MAX / 7);
  RC_TRY(stage_check_max_edges("lbmdem_geodesic_compute", max_edges));
  RC_TRY(stage_check_map("lbmdem_geodesic_compute", map, lx, ly, n));
  // min_d2 > 1: the clearance first; the result of the handle's map is reused while its guard calls it valid
  const auto& Q = h->clr;
  const bool narrow = min_d2 > 1;
  if (narrow && (map || !(Q.at.current(h) && Q.own))) {
    long cc[LBMDEM_CLEARANCE_COUNTS];
    RC_TRY(lbmdem_clearance_compute(h, map, max_edges, cc));
  }
  RC_TRY(geodesic_stage(h));
  const hipStream_t st = h->stream;
  const long N = (long)lx * sy;
  GeoJob J{};
  if (narrow) J.d2 = Q.d2;
  else if (map) {
    RC_TRY(stage_upload_map(h, &V.map, map));
    J.M = V.map;
  } else J.M = reader_obst(h);
  J.min_d2 = min_d2;
  J.lx = lx; J.ly = ly; J.sy = sy; J.conn = conn;
  J.band = band < GEO_SIDE_MAX ? band : GEO_SIDE_MAX;   // (the sides are clamped to the lattice)
  J.from = from; J.to = to;
  J.N = N;
  J.ntx = (int)stage_blocks(lx, GEO_TX); J.nty = (int)stage_blocks(ly, GEO_TY);
  J.dist = V.dist; J.back = V.back; J.detour = V.detour;
  J.stamp = V.stamp;
  J.words = V.words;
  const int nd = geo_depthmax(lx, ly, from) + 1;
  HIP_TRY(h->mem.grow(&V.lev, &V.lev_cap, 3 * (long)nd));
  HIP_TRY(h->mem.grow(&V.lmm, &V.lmm_cap, 2 * (long)nd));
  J.lev = V.lev; J.lmin = V.lmm; J.lmax = V.lmm + nd; J.nd = nd;
  HIP_TRY(hipMemsetAsync(V.words, 0, sizeof(geo_u64) * GEO_WORDS, st));
  HIP_TRY(hipMemsetAsync(V.words + GEO_W_SHORTEST, 0xFF, sizeof(geo_u64), st));
  HIP_TRY(hipMemsetAsync(V.lev, 0, sizeof(geo_u64) * 3 * (size_t)nd, st));
  HIP_TRY(hipMemsetAsync(J.lmin, 0x7F, sizeof(int) * (size_t)nd, st));
  HIP_TRY(hipMemsetAsync(J.lmax, 0xFF, sizeof(int) * (size_t)nd, st));
  V.rounds[0] = V.rounds[1] = 0;
  RC_TRY(geodesic_pass(h, J, V.dist, from, GEO_W_FLUID, &V.rounds[0]));   // (synchronises: the caller's map has been read)
  if (to) RC_TRY(geodesic_pass(h, J, V.back, to, GEO_W_BACK0, &V.rounds[1]));
  else HIP_TRY(hipMemsetAsync(V.back, 0xFF, sizeof(int) * (size_t)N, st));
  hipLaunchKernelGGL(k_geo_finish, dim3((unsigned)stage_blocks(sy, GEO_THREADS), (unsigned)stage_blocks(lx, GEO_ROWS)), dim3(GEO_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_geo_detour, dim3((unsigned)stage_blocks(N, GEO_THREADS)), dim3(GEO_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[GEO_WORDS] = {};
  std::vector<unsigned long long> lev(3 * (size_t)nd);
  std::vector<int> lmm(2 * (size_t)nd);
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(lev.data(), V.lev, sizeof(geo_u64) * lev.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(lmm.data(), V.lmm, sizeof(int) * lmm.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const bool through = w[GEO_W_SHORTEST] != ~0ull;
  counts10[0] = (long)w[GEO_W_FLUID];
  counts10[1] = (long)w[GEO_W_PASSABLE];
  counts10[2] = (long)w[GEO_W_INLET];
  counts10[3] = (long)w[GEO_W_REACHED];
  counts10[4] = (long)w[GEO_W_MAX] - 1;
  counts10[5] = (long)w[GEO_W_OUTLET];
  counts10[6] = (long)w[GEO_W_OUTLET_REACHED];
  counts10[7] = through ? (long)(w[GEO_W_SHORTEST] >> 32) : -1;
  counts10[8] = through ? (long)(w[GEO_W_SHORTEST] & 0xFFFFFFFFull) : -1;
  counts10[9] = (long)w[GEO_W_PATH];
  V.levels.resize((size_t)nd);
  for (int k = 0; k < nd; ++k) {
    lbmdem_geo_level& e = V.levels[(size_t)k];
    e.nodes = (long)lev[(size_t)k]; e.reached = (long)lev[(size_t)nd + k]; e.sum = (long)lev[2 * (size_t)nd + k];
    e.dmin = e.reached ? lmm[(size_t)k] : -1;
    e.dmax = e.reached ? lmm[(size_t)nd + k] : -1;
  }
  V.over_clearance = narrow && !map;
  V.gen = Q.gen;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_geodesic(lbmdem_handle* h, int* dist, int* back, int* detour) try {
  CHECK_H(h);
  RC_TRY(geodesic_ready(h, "lbmdem_download_geodesic"));
  int* const out[3] = {dist, back, detour};
  const int* const src[3] = {h->geo.dist, h->geo.back, h->geo.detour};
  for (int k = 0; k < 3; ++k)
    if (out[k]) RC_TRY(stage_download_plane(h, out[k], src[k]));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_geodesic_device(lbmdem_handle* h, const int** dist, const int** back, const int** detour, int* sy) try {
  CHECK_H(h);
  if (!dist || !back || !detour || !sy) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(geodesic_ready(h, "lbmdem_geodesic_device"));
  *dist = h->geo.dist;
  *back = h->geo.back;
  *detour = h->geo.detour;
  *sy = h->L.sy;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_geodesic_profile(lbmdem_handle* h, lbmdem_geo_level* rec, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !rec)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(geodesic_ready(h, "lbmdem_download_geodesic_profile"));
  const auto& lv = h->geo.levels;   // (on the host already: not a stage_table)
  const long have = (long)lv.size();
  *count = have;
  if (cap == 0) return LBMDEM_OK;   // (how many there are)
  if (cap < have) return fail(LBMDEM_EINVAL, "lbmdem_download_geodesic_profile: there are %ld depths, the buffer holds %ld", have, cap);
  for (long k = 0; k < have; ++k) rec[k] = lv[(size_t)k];
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_geodesic_rounds(lbmdem_handle* h, int* fwd, int* bwd) try {
  CHECK_H(h);
  if (!fwd || !bwd) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(geodesic_ready(h, "lbmdem_geodesic_rounds"));
  *fwd = h->geo.rounds[0];
  *bwd = h->geo.rounds[1];
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_geodesic(lbmdem_handle* h, const char* dir, int nfile, int from, int band, int to, int conn, int min_d2, int plane) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_geodesic"));
  const LatticeView& L = h->L;
  long counts[LBMDEM_GEODESIC_COUNTS];
  RC_TRY(lbmdem_geodesic_compute(h, nullptr, from, band, to, conn, min_d2, 0, counts));
  const size_t cnt = plane ? (size_t)L.lx * L.ly : 0;
  std::vector<int> dist(cnt), back(cnt), detour(cnt);
  if (plane) RC_TRY(lbmdem_download_geodesic(h, dist.data(), back.data(), detour.data()));
  const auto& lv = h->geo.levels;
  return lbmdem_write_geodesic_files(dir, nfile, L.lx, L.ly, h->n, from, band, to, conn, min_d2, plane, plane ? dist.data() : nullptr,
                                     plane ? back.data() : nullptr, plane ? detour.data() : nullptr, lv.data(), (long)lv.size(), counts,
                                     h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_geodesic_output(lbmdem_handle* h, int on, int from, int band, int to, int conn, int min_d2, int plane) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_geodesic_output"));
    RC_TRY(geodesic_args("lbmdem_set_geodesic_output", from, band, to, conn, min_d2));
    h->geodesic_from = from; h->geodesic_band = band; h->geodesic_to = to;
    h->geodesic_conn = conn; h->geodesic_min_d2 = min_d2;
    h->geodesic_plane = plane != 0;
  }
  h->geodesic_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
