// lbm_pores.hip -- is the pore space connected: the fluid phase of the obstacle map labelled into connected components, per
// component its size, extent, walls, wetted links and fluid mass, per grain the pores it borders (lbmdem_pore_compute,
// lbmdem_download_pore_labels, lbmdem_pore_labels_device, lbmdem_download_pores, lbmdem_download_pore_grains,
// lbmdem_pore_grains_device, lbmdem_write_pores, lbmdem_set_pores_output, lbmdem_write_pore_files; include/lbmdem_hip.h has the
// contract in full). Every result is an integer and the labels are canonical -- the smallest node of a component -- so nothing
// depends on the order anything happens in. Nothing here is on the step path: the kernels only read the map and f and write to
// the handle's PoreStage, and nothing is allocated or launched before the first compute.
//
// A union-find over the lattice in the device layout (node = x*sy + y: the same order as the host's index x*ly + y, so the
// smallest device node of a component is its smallest host index). parent[node] is a node of the same component that is no larger
// than the node itself, -1 off the fluid. That one invariant carries everything: a find walks strictly downward and ends within
// `node` steps whatever other lanes do meanwhile, no cycle can form, and the root of a finished component is its smallest node.
// A union hooks the larger of two roots below the smaller with atomicMin and starts again from what it found there only when
// another lane has lowered that root first (the sum of the two nodes falls with every retry). A stale read of a parent is a
// former parent: still a smaller node of the same component.
// On the handle's stream:
//   k_po_local    one workgroup per tile of 16 x 64 nodes, lanes along y. The tile's parents live in LDS; every fluid node is
//                 united with its four neighbours of smaller index inside the tile (two when conn == 4), then stores the
//                 device node of its LDS root: per fluid node a parent that already is the tile's smallest node of its component;
//   k_po_seam     one lane per node on a tile border: the same unions across the seams, in global memory;
//   k_po_flatten  every fluid node is set to its root; the roots (parent == node) are counted per block of 1024 nodes;
//   a scan        over the blocks' counts;
//   k_po_emit     a block scan ranks the block's roots in node order: rank[root], and the root's table entry is started;
//   k_po_table    lanes along y, 32 rows per workgroup: a node's eight neighbours, its rho; the lanes of a wavefront that
//                 share a label (or a grain) are summed towards the first of them by shifts, the workgroup's first label gathers
//                 in an LDS slot, and what remains goes to the table through the rank with 64-bit integer atomics, atomicMin and
//                 atomicMax -- the one big pore would serialise every node on one address otherwise. The grain outputs come
//                 from the grain nodes of the same pass. The label plane in host indices is written here;
//   k_po_census, k_po_grains   the counts over the table and over the grains.
// Single launches, no host-driven rounds: a serpentine pore would need thousands. No workgroup waits for another; every loop has
// the bound its comment states. No floating-point atomics.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h), MemPool (lbm_mem.h) for the
// scratch kept on the handle, OutFile (lbm_outfile.h) for the files; what the pore stages share, lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

constexpr long PO_NODES_MAX = (long)1 << 31;   // labels are int

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int PO_TX = 16, PO_TY = 64;          // a tile: rows (x) and columns (y, the contiguous axis)
constexpr int PO_TILE = PO_TX * PO_TY;
constexpr int PO_THREADS = 256;
constexpr int PO_BLOCK_NODES = 4 * PO_THREADS;   // nodes of a block of the flatten and emit passes: four per lane, one 16-byte load
constexpr int PO_ROWS = 32;                    // rows of a workgroup of the table pass
constexpr double PO_Q32 = 4294967296.;
constexpr double PO_RHO_MAX = 1048576.;        // 2^20
// PoreStage::words
enum : int { PO_W_FLUID = 0, PO_W_SKIPPED, PO_W_LARGEST, PO_W_SINGLE, PO_W_SPAN, PO_W_THROAT, PO_W_DRY, PO_WORDS };

struct PoJob {
  const int* M;      // the map, device layout
  const real* f;
  int lx, ly, sy, n, conn;
  long N;            // lx * sy
  int* parent;
  int* label;
  int* rank;
  int* cnt;          // [nblocks + 1] roots per block
  int* off;          // [nblocks + 1] their scan
  int nblocks;
  lbmdem_pore* table;
  long ncomp;
  int *wet, *pmin, *pmax;
  unsigned long long* words;
};

// The root of `a`. parent[v] <= v and only a root has parent[v] == v: the walk falls strictly and ends within `a` steps. (A node
// off the fluid has -1 and is never handed in; the test only keeps an index inside the array.)
__device__ __forceinline__ int po_find_lds(volatile int* p, int a) {
  for (int b = p[a]; b != a && b >= 0; b = p[a]) a = b;
  return a;
}
__device__ __forceinline__ int po_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int po_find(const int* p, int a) {
  for (int b = po_load(p + a); b != a && b >= 0; b = po_load(p + a)) a = b;
  return a;
}
// The components of a and b become one. Every retry starts from a node below the root it failed on: at most a + b rounds.
__device__ __forceinline__ void po_union_lds(int* p, int a, int b) {
  for (;;) {
    a = po_find_lds(p, a); b = po_find_lds(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }   // a: the larger root
    const int old = atomicMin(&p[a], b);
    if (old == a) return;   // a was a root still: hooked
    a = old;                // another lane has lowered it to `old`, of the same component as a: unite that with b
  }
}
__device__ __forceinline__ void po_union(int* p, int a, int b) {
  for (;;) {
    a = po_find(p, a); b = po_find(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&p[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(PO_THREADS) void k_po_local(const PoJob J) {
  __shared__ int p[PO_TILE];
  const int ty = threadIdx.x & (PO_TY - 1), tx0 = threadIdx.x / PO_TY;   // four rows per lane: tx0, tx0 + 4, ..
  const int x0 = blockIdx.y * PO_TX, y0 = blockIdx.x * PO_TY;
  const int y = y0 + ty;
#pragma unroll
  for (int k = 0; k < PO_TX / 4; ++k) {
    const int tx = tx0 + 4 * k, x = x0 + tx;
    const bool fluid = x < J.lx && y < J.ly && J.M[(long)x * J.sy + y] == -1;
    p[tx * PO_TY + ty] = fluid ? tx * PO_TY + ty : -1;
  }
  __syncthreads();
  const bool diag = J.conn == 8;
#pragma unroll
  for (int k = 0; k < PO_TX / 4; ++k) {
    const int tx = tx0 + 4 * k, me = tx * PO_TY + ty;
    if (p[me] < 0) continue;
    // the neighbours of smaller index inside the tile: (x, y-1), (x-1, y-1), (x-1, y), (x-1, y+1)
    if (ty > 0 && p[me - 1] >= 0) po_union_lds(p, me, me - 1);
    if (tx > 0) {
      if (p[me - PO_TY] >= 0) po_union_lds(p, me, me - PO_TY);
      if (diag && ty > 0 && p[me - PO_TY - 1] >= 0) po_union_lds(p, me, me - PO_TY - 1);
      if (diag && ty + 1 < PO_TY && p[me - PO_TY + 1] >= 0) po_union_lds(p, me, me - PO_TY + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PO_TX / 4; ++k) {
    const int tx = tx0 + 4 * k, x = x0 + tx, me = tx * PO_TY + ty;
    if (x >= J.lx || y >= J.sy) continue;   // (the pad columns ly .. sy - 1 take -1)
    int out = -1;
    if (p[me] >= 0) {
      const int r = po_find_lds(p, me);
      out = (x0 + r / PO_TY) * J.sy + y0 + (r & (PO_TY - 1));
    }
    J.parent[(long)x * J.sy + y] = out;
  }
}

// The unions across the tiles' borders. An edge from (x, y) to a neighbour of smaller index crosses a border when x is the first
// row of a tile (the three neighbours in row x - 1), when y is the first column of a tile ((x, y-1) and (x-1, y-1)) or when y is
// the last column of one ((x-1, y+1)). part 0: the lanes run along the first rows of the tiles, blockIdx.y the tile row (from the
// second on); part 1: blockIdx.y the seam between two tile columns, its last and first column, the lanes run along x.
// Most of these edges say nothing new, and in one big pore every union that is tried lands on the same few roots:
//  - a diagonal edge is left out where one of the other two nodes of its square is fluid: that node has an axis edge to either end
//    (inside a tile, or across a seam where this kernel makes it), so the ends are joined without it;
//  - an axis edge is left out where the lane before makes the same union: its two nodes have the same two parents. Two nodes with
//    one parent are of one component, now and later, so whichever lane of such a run does not leave its edge out -- the first
//    at the latest -- joins the same two components. (Only roots are lowered while this kernel runs, and a lowered root still is
//    of the same component.)
__global__ __launch_bounds__(PO_THREADS) void k_po_seam(const PoJob J, const int part) {
  const bool diag = J.conn == 8;
  int* const P = J.parent;
  const int sy = J.sy;
  if (part == 0) {
    const int x = (blockIdx.y + 1) * PO_TX, y = blockIdx.x * PO_THREADS + threadIdx.x;
    if (x >= J.lx || y >= J.ly) return;
    const int me = x * sy + y;
    const int pm = P[me];
    if (pm < 0) return;
    const int up = me - sy;
    const int pu = P[up];
    if (pu >= 0) {
      if (!(y > 0 && P[me - 1] == pm && P[up - 1] == pu)) po_union(P, me, up);
    } else if (diag) {
      if (y > 0 && P[me - 1] < 0 && P[up - 1] >= 0) po_union(P, me, up - 1);
      if (y + 1 < J.ly && P[me + 1] < 0 && P[up + 1] >= 0) po_union(P, me, up + 1);
    }
  } else {
    const int x = blockIdx.x * PO_THREADS + threadIdx.x;
    const int y1 = ((blockIdx.y >> 1) + 1) * PO_TY;   // the first column of the tiles right of the seam
    if (x >= J.lx || y1 >= J.ly) return;
    if (blockIdx.y & 1) {
      const int me = x * sy + y1;
      const int pm = P[me];
      if (pm < 0) return;
      const int pl = P[me - 1];
      if (pl >= 0) {
        if (!(x > 0 && P[me - sy] == pm && P[me - sy - 1] == pl)) po_union(P, me, me - 1);
      } else if (diag && x > 0 && P[me - sy] < 0 && P[me - sy - 1] >= 0) {
        po_union(P, me, me - sy - 1);
      }
    } else {
      const int me = x * sy + y1 - 1;
      if (P[me] < 0) return;
      if (diag && x > 0 && P[me + 1] < 0 && P[me - sy] < 0 && P[me - sy + 1] >= 0) po_union(P, me, me - sy + 1);
    }
  }
}

__device__ __forceinline__ int po_wave_sum(int v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}

// Every fluid node takes its root; the block's roots are counted. Four consecutive nodes per lane (lx * sy is a multiple of 16).
__global__ __launch_bounds__(PO_THREADS) void k_po_flatten(const PoJob J) {
  __shared__ int part[PO_THREADS / 64];
  const long node0 = ((long)blockIdx.x * PO_THREADS + threadIdx.x) * 4;
  int roots = 0;
  if (node0 < J.N) {
    int4 v = *reinterpret_cast<const int4*>(J.parent + node0);
    int* const c = reinterpret_cast<int*>(&v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c[k] >= 0) {
        c[k] = po_find(J.parent, c[k]);
        roots += c[k] == (int)(node0 + k);
      }
    *reinterpret_cast<int4*>(J.parent + node0) = v;   // (a lane that walks through here meanwhile finds a root: a smaller node of the component)
  }
  roots = po_wave_sum(roots);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < PO_THREADS / 64; ++w) s += part[w];
    J.cnt[blockIdx.x] = s;
    if (blockIdx.x == 0) J.cnt[J.nblocks] = 0;   // the scan's last item
  }
}

// The roots in node order: rank[root] = its place in the table, whose entry starts empty.
__global__ __launch_bounds__(PO_THREADS) void k_po_emit(const PoJob J) {
  typedef hipcub::BlockScan<int, PO_THREADS> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const long node0 = ((long)blockIdx.x * PO_THREADS + threadIdx.x) * 4;
  int4 v = make_int4(-1, -1, -1, -1);
  if (node0 < J.N) v = *reinterpret_cast<const int4*>(J.parent + node0);
  const int* const c = reinterpret_cast<const int*>(&v);
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) mine += c[k] >= 0 && c[k] == (int)(node0 + k);
  int before = 0;
  Scan(tmp).ExclusiveSum(mine, before);
  long at = (long)J.off[blockIdx.x] + before;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (c[k] < 0 || c[k] != (int)(node0 + k)) continue;
    if (at < J.ncomp) {   // (always: ncomp is the scan's total)
      const int nd = c[k];
      J.rank[nd] = (int)at;
      lbmdem_pore e;
      e.label = (nd / J.sy) * J.ly + nd % J.sy;
      e.walls = 0;
      e.nodes = 0; e.grain_links = 0; e.wall_links = 0; e.mass_q32 = 0;
      e.xmin = INT_MAX; e.xmax = -1; e.ymin = INT_MAX; e.ymax = -1;
      J.table[at] = e;
    }
    ++at;
  }
}

__global__ __launch_bounds__(PO_THREADS) void k_po_init(const PoJob J) {
  const int i = blockIdx.x * PO_THREADS + threadIdx.x;
  if (i < J.n) { J.wet[i] = 0; J.pmin[i] = INT_MAX; J.pmax[i] = -1; }
  if (i < PO_WORDS) J.words[i] = 0;
}

// one component's share of a wavefront, a workgroup or a node into its table entry
struct PoShare {
  unsigned long long nodes, glinks, wlinks, mass;
  int walls, xmin, xmax, ymin, ymax;
};
__device__ __forceinline__ void po_table_add(lbmdem_pore* e, const PoShare& s) {
  atomicAdd(reinterpret_cast<unsigned long long*>(&e->nodes), s.nodes);
  if (s.glinks) atomicAdd(reinterpret_cast<unsigned long long*>(&e->grain_links), s.glinks);
  if (s.wlinks) atomicAdd(reinterpret_cast<unsigned long long*>(&e->wall_links), s.wlinks);
  if (s.mass) atomicAdd(reinterpret_cast<unsigned long long*>(&e->mass_q32), s.mass);
  // a look first: these only ever move one way, so a value seen that leaves nothing to do is a reason not to ask
  if (s.walls & ~po_load(&e->walls)) atomicOr(&e->walls, s.walls);
  if (s.xmin < po_load(&e->xmin)) atomicMin(&e->xmin, s.xmin);
  if (s.xmax > po_load(&e->xmax)) atomicMax(&e->xmax, s.xmax);
  if (s.ymin < po_load(&e->ymin)) atomicMin(&e->ymin, s.ymin);
  if (s.ymax > po_load(&e->ymax)) atomicMax(&e->ymax, s.ymax);
}

__global__ __launch_bounds__(PO_THREADS) void k_po_table(const PoJob J) {
  // the slot of the workgroup's first label
  __shared__ int s_key, s_walls, s_box[4];
  __shared__ unsigned long long s_sum[4], s_seen[2];   // s_seen: the workgroup's fluid nodes, and those of them whose rho was left out
  if (threadIdx.x == 0) {
    s_key = -1; s_walls = 0;
    s_seen[0] = s_seen[1] = 0;
    s_box[0] = INT_MAX; s_box[1] = -1; s_box[2] = INT_MAX; s_box[3] = -1;
    s_sum[0] = s_sum[1] = s_sum[2] = s_sum[3] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * PO_THREADS + threadIdx.x;
  const int lx = J.lx, ly = J.ly, sy = J.sy, n = J.n;
  unsigned long long nfluid = 0, nskipped = 0;   // of the wavefront, over its rows (every lane holds the same)
  for (int r = 0; r < PO_ROWS; ++r) {
    const int x = blockIdx.y * PO_ROWS + r;
    if (x >= lx) break;   // (the whole workgroup)
    const long node = (long)x * sy + y;
    const int m = y < ly ? J.M[node] : n;
    // key: the root of a fluid node, -2 - i on grain i, -1 where there is nothing to add
    int key = -1;
    int s0 = 0, s1 = 0, walls = 0, mn = INT_MAX, mx = -1;
    long long mass = 0;
    bool skipped = false;
    if (m == -1) {
      key = J.parent[node];
#pragma unroll
      for (int q = 1; q <= 8; ++q) {
        const int nx = x + EXq(q), ny = y + EYq(q);
        const bool outside = nx < 0 || nx >= lx || ny < 0 || ny >= ly;
        const int mm = outside ? n : J.M[(long)nx * sy + ny];
        if (mm == n) {
          ++s1;
          walls |= (ny <= 0 ? 1 : 0) | (ny >= ly - 1 ? 2 : 0) | (nx <= 0 ? 4 : 0) | (nx >= lx - 1 ? 8 : 0);
        } else if (mm >= 0) {
          ++s0;
        }
      }
      double rho = 0.;
      const long fb = fbase(node);
#pragma unroll
      for (int q = 0; q < 9; ++q) rho += J.f[fb + q * LBMDEM_TILE_Y];
      if (fabs(rho) < PO_RHO_MAX) mass = __double2ll_rn(rho * PO_Q32);   // (false for a NaN and an infinity)
      else skipped = true;
    } else if (m >= 0 && m < n) {
#pragma unroll
      for (int q = 1; q <= 8; ++q) {
        const int nx = x + EXq(q), ny = y + EYq(q);
        if (nx < 0 || nx >= lx || ny < 0 || ny >= ly) continue;
        const long nn = (long)nx * sy + ny;
        if (J.M[nn] != -1) continue;
        const int root = J.parent[nn];
        const int lab = (root / sy) * ly + root % sy;
        ++s0;
        mn = lab < mn ? lab : mn;
        mx = lab > mx ? lab : mx;
      }
      if (s0 > 0) key = -2 - m;
    }
    if (y < sy) J.label[node] = m == -1 ? (key / sy) * ly + key % sy : -1;
    // runs of one key along the lanes, summed towards their first lane: after the step of d a lane holds what the lanes up to
    // 2d - 1 further on in its run have, and a lane d further on is of the same run exactly when everything between is
    const int before = __shfl_up(key, 1);
    const bool head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & ((2ull << lane) - 1ull));
    unsigned long long massu = (unsigned long long)mass;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o_run = __shfl_down(run, d);
      const int o0 = __shfl_down(s0, d), o1 = __shfl_down(s1, d), ow = __shfl_down(walls, d);
      const int omn = __shfl_down(mn, d), omx = __shfl_down(mx, d);
      const unsigned long long om = __shfl_down(massu, d);
      if (lane + d < 64 && o_run == run) {
        s0 += o0; s1 += o1; walls |= ow; massu += om;
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
      }
    }
    const unsigned long long later = lane < 63 ? heads >> (lane + 1) : 0ull;
    const int len = later ? __ffsll((long long)later) : 64 - lane;   // lanes of the run
    nskipped += __popcll(__ballot(skipped));
    nfluid += __popcll(__ballot(m == -1));
    if (head && key >= 0) {
      const int held = atomicCAS(&s_key, -1, key);
      if (held == -1 || held == key) {
        atomicAdd(&s_sum[0], (unsigned long long)len);
        if (s0) atomicAdd(&s_sum[1], (unsigned long long)s0);
        if (s1) atomicAdd(&s_sum[2], (unsigned long long)s1);
        if (massu) atomicAdd(&s_sum[3], massu);
        if (walls) atomicOr(&s_walls, walls);
        atomicMin(&s_box[0], x); atomicMax(&s_box[1], x);
        atomicMin(&s_box[2], y); atomicMax(&s_box[3], y + len - 1);
      } else {
        PoShare s;
        s.nodes = (unsigned long long)len; s.glinks = (unsigned long long)s0; s.wlinks = (unsigned long long)s1; s.mass = massu;
        s.walls = walls; s.xmin = x; s.xmax = x; s.ymin = y; s.ymax = y + len - 1;
        po_table_add(J.table + J.rank[key], s);
      }
    } else if (head && key <= -2) {
      const int i = -2 - key;
      atomicAdd(&J.wet[i], s0);
      if (mn < po_load(&J.pmin[i])) atomicMin(&J.pmin[i], mn);
      if (mx > po_load(&J.pmax[i])) atomicMax(&J.pmax[i], mx);
    }
  }
  if (lane == 0) {
    if (nfluid) atomicAdd(&s_seen[0], nfluid);
    if (nskipped) atomicAdd(&s_seen[1], nskipped);
  }
  __syncthreads();
  // (one atomic per workgroup and word: a quarter of a million of them on one address take milliseconds)
  if (threadIdx.x == 0 && s_seen[0]) atomicAdd(&J.words[PO_W_FLUID], s_seen[0]);
  if (threadIdx.x == 0 && s_seen[1]) atomicAdd(&J.words[PO_W_SKIPPED], s_seen[1]);
  if (threadIdx.x == 0 && s_key >= 0) {
    PoShare s;
    s.nodes = s_sum[0]; s.glinks = s_sum[1]; s.wlinks = s_sum[2]; s.mass = s_sum[3];
    s.walls = s_walls; s.xmin = s_box[0]; s.xmax = s_box[1]; s.ymin = s_box[2]; s.ymax = s_box[3];
    po_table_add(J.table + J.rank[s_key], s);
  }
}

// The largest component (the smallest label among equals: nodes in the high bits, the label's complement below), the components
// of one node, the spanning mask.
__global__ __launch_bounds__(PO_THREADS) void k_po_census(const PoJob J) {
  const long k = (long)blockIdx.x * PO_THREADS + threadIdx.x;
  unsigned long long best = 0;
  bool single = false;
  int span = 0;
  if (k < J.ncomp) {
    const lbmdem_pore e = J.table[k];
    best = ((unsigned long long)e.nodes << 31) | (unsigned long long)(INT_MAX - e.label);
    single = e.nodes == 1;
    span = ((e.walls & 12) == 12 ? 1 : 0) | ((e.walls & 3) == 3 ? 2 : 0);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m);
    best = o > best ? o : best;
    span |= __shfl_xor(span, m);
  }
  const unsigned long long singles = __popcll(__ballot(single));
  if ((threadIdx.x & 63) == 0) {
    if (best) atomicMax(&J.words[PO_W_LARGEST], best);
    if (singles) atomicAdd(&J.words[PO_W_SINGLE], singles);
    if (span) atomicOr(&J.words[PO_W_SPAN], (unsigned long long)span);
  }
}

__global__ __launch_bounds__(PO_THREADS) void k_po_grains(const PoJob J) {
  const int i = blockIdx.x * PO_THREADS + threadIdx.x;
  bool throat = false, dry = false;
  if (i < J.n) {
    int mn = J.pmin[i];
    if (mn == INT_MAX) J.pmin[i] = mn = -1;
    throat = mn != J.pmax[i];
    dry = J.wet[i] == 0;
  }
  const unsigned long long nt = __popcll(__ballot(throat)), nd = __popcll(__ballot(dry));
  if ((threadIdx.x & 63) == 0) {
    if (nt) atomicAdd(&J.words[PO_W_THROAT], nt);
    if (nd) atomicAdd(&J.words[PO_W_DRY], nd);
  }
}

// what depends on the lattice and on n, once
int pore_stage(lbmdem_handle* h) {
  auto& V = h->po;
  if (V.words) return LBMDEM_OK;
  const size_t N = (size_t)h->L.lx * h->L.sy;
  const int nb = (int)stage_blocks((long)N, PO_BLOCK_NODES);
  HIP_TRY(h->mem.dev(&V.parent, N));
  HIP_TRY(h->mem.dev(&V.label, N));
  HIP_TRY(h->mem.dev(&V.rank, N));
  HIP_TRY(h->mem.dev(&V.cnt, 2 * ((size_t)nb + 1)));
  HIP_TRY(h->mem.dev(&V.grains, 3 * (size_t)h->n));
  size_t b = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int*)nullptr, (int*)nullptr, nb + 1, h->stream));
  HIP_TRY(h->mem.grow(&V.tmp, &V.tmp_bytes, (long)b));
  HIP_TRY(h->mem.dev(&V.words, (size_t)PO_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

int pores_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  if (!h->po.at.current(h))
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_pore_compute has been made for the map and the populations as they are now", who);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_pore_files(const char* dir, int nfile, int conn, int lx, int ly, int plane, const int* label,
                            const lbmdem_pore* table, long ntable, int n, const int* wet, const int* pore_min,
                            const int* pore_max, const long* counts10, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || ntable < 0 || (ntable > 0 && !table) || !wet || !pore_min || !pore_max || !counts10 || (plane && !label))
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_pore_files arguments");
  if (conn != 4 && conn != 8) return fail(LBMDEM_EINVAL, "lbmdem_write_pore_files: conn is 4 or 8 (%d)", conn);
  if (lx < 2 || ly < 2 || (long)lx * ly >= PO_NODES_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_pore_files: the lattice is %d x %d", lx, ly);
  const long cnt = (long)lx * ly;
  if (label)
    for (long k = 0; k < cnt; ++k)
      if (label[k] < -1 || label[k] >= cnt)
        return fail(LBMDEM_EINVAL, "lbmdem_write_pore_files: label[%ld][%ld] = %d is outside [-1, %ld)", k / ly, k % ly, label[k], cnt);
  for (long k = 0; k < ntable; ++k)
    if (table[k].label < 0 || table[k].label >= cnt || (k > 0 && table[k].label <= table[k - 1].label))
      return fail(LBMDEM_EINVAL, "lbmdem_write_pore_files: entry %ld of the table has the label %d: the labels ascend inside [0, %ld)",
                  k, table[k].label, cnt);
  OutFile F;
  RC_TRY(F.open("w", dir, "pore_table%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# conn %d lx %d ly %d\n", conn, lx, ly);
  fprintf(fp, "# label nodes xmin xmax ymin ymax grain_links wall_links walls mass_q32\n");
  for (long k = 0; k < ntable; ++k) {
    const lbmdem_pore& e = table[k];
    fprintf(fp, "%d %ld %d %d %d %d %ld %ld %d %ld\n", e.label, e.nodes, e.xmin, e.xmax, e.ymin, e.ymax, e.grain_links, e.wall_links,
            e.walls, e.mass_q32);
  }
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "pore_grains%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# i wet pore_min pore_max\n");
  for (int i = 0; i < n; ++i) fprintf(fp, "%d %d %d %d\n", i, wet[i], pore_min[i], pore_max[i]);
  RC_TRY(F.close());
  if (plane) {
    const char* const names[1] = {"pore"};
    // (this file alone ends with its plane's last byte, no line feed behind it)
    RC_TRY(stage_write_int_planes(F, dir, nfile, "pores%.6i.vtk", "lbmdem pore labels", lx, ly, names, &label, 1, false));
  }
  return stage_append_row(F, dir, "pores.data",
                          "# t fluid_nodes components largest_nodes largest_label trapped_nodes single_nodes spanning throat_grains "
                          "dry_grains unaccumulated", t, counts10, LBMDEM_PORE_COUNTS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_pore_compute(lbmdem_handle* h, int, const int*, long*) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_download_pore_labels(lbmdem_handle* h, int*) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_pore_labels_device(lbmdem_handle* h, const int**, int*) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_download_pores(lbmdem_handle* h, lbmdem_pore*, long, long*) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_download_pore_grains(lbmdem_handle* h, int*, int*, int*) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_pore_grains_device(lbmdem_handle* h, const int**, const int**, const int**) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_write_pores(lbmdem_handle* h, const char*, int, int, int) { SP_REFUSE(h, "the pore space analysis"); }
int lbmdem_set_pores_output(lbmdem_handle* h, int, int, int) { SP_REFUSE(h, "the pore space analysis"); }
#else

int lbmdem_pore_compute(lbmdem_handle* h, int conn, const int* map, long* counts10) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_pore_compute"));
  if (conn != 4 && conn != 8) return fail(LBMDEM_EINVAL, "lbmdem_pore_compute: conn is 4 or 8 (%d)", conn);
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  if ((long)lx * ly >= PO_NODES_MAX || (long)lx * sy >= PO_NODES_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_pore_compute: a lattice of %d x %d nodes (row pitch %d) has 2^31 nodes or more: the labels "
                               "are 32-bit integers", lx, ly, sy);
  auto& V = h->po;
  V.at.valid = false;
  RC_TRY(stage_check_map("lbmdem_pore_compute", map, lx, ly, n));
  RC_TRY(pore_stage(h));
  const hipStream_t st = h->stream;
  const long N = (long)lx * sy;
  PoJob J{};
  J.M = reader_obst(h);
  if (map) {
    RC_TRY(stage_upload_map(h, &V.map, map));
    J.M = V.map;
  }
  J.f = h->f[h->fcur];
  J.lx = lx; J.ly = ly; J.sy = sy; J.n = n; J.conn = conn;
  J.N = N;
  J.parent = V.parent; J.label = V.label; J.rank = V.rank;
  J.nblocks = (int)stage_blocks(N, PO_BLOCK_NODES);
  J.cnt = V.cnt; J.off = V.cnt + J.nblocks + 1;
  J.wet = V.grains; J.pmin = V.grains + n; J.pmax = V.grains + 2 * (size_t)n;
  J.words = V.words;
  const int need = n > PO_WORDS ? n : PO_WORDS;
  hipLaunchKernelGGL(k_po_init, dim3((unsigned)stage_blocks(need, PO_THREADS)), dim3(PO_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_po_local, dim3((unsigned)stage_blocks(ly, PO_TY), (unsigned)stage_blocks(lx, PO_TX)), dim3(PO_THREADS), 0, st, J);
  if (lx > PO_TX)
    hipLaunchKernelGGL(k_po_seam, dim3((unsigned)stage_blocks(ly, PO_THREADS), (lx - 1) / PO_TX), dim3(PO_THREADS), 0, st, J, 0);
  if (ly > PO_TY)
    hipLaunchKernelGGL(k_po_seam, dim3((unsigned)stage_blocks(lx, PO_THREADS), 2 * ((ly - 1) / PO_TY)), dim3(PO_THREADS), 0, st, J, 1);
  hipLaunchKernelGGL(k_po_flatten, dim3(J.nblocks), dim3(PO_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  size_t bytes = (size_t)V.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(V.tmp, bytes, J.cnt, J.off, J.nblocks + 1, st));
  int ncomp = 0;
  HIP_TRY(hipMemcpyAsync(&ncomp, J.off + J.nblocks, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // (the caller's map has been read too)
  if (ncomp > 0) HIP_TRY(h->mem.grow(&V.table, &V.table_cap, (long)ncomp + ncomp / 4 + 64));
  J.table = V.table; J.ncomp = ncomp;
  if (ncomp > 0) {
    hipLaunchKernelGGL(k_po_emit, dim3(J.nblocks), dim3(PO_THREADS), 0, st, J);
  }
  hipLaunchKernelGGL(k_po_table, dim3((unsigned)stage_blocks(sy, PO_THREADS), (unsigned)stage_blocks(lx, PO_ROWS)), dim3(PO_THREADS), 0, st, J);
  if (ncomp > 0) hipLaunchKernelGGL(k_po_census, dim3((unsigned)stage_blocks(ncomp, PO_THREADS)), dim3(PO_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_po_grains, dim3((unsigned)stage_blocks(n, PO_THREADS)), dim3(PO_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[PO_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const long largest = (long)(w[PO_W_LARGEST] >> 31);
  counts10[0] = (long)w[PO_W_FLUID];
  counts10[1] = ncomp;
  counts10[2] = largest;
  counts10[3] = ncomp > 0 ? (long)(INT_MAX - (int)(w[PO_W_LARGEST] & 0x7FFFFFFFull)) : -1;
  counts10[4] = counts10[0] - largest;
  counts10[5] = (long)w[PO_W_SINGLE];
  counts10[6] = (long)w[PO_W_SPAN];
  counts10[7] = (long)w[PO_W_THROAT];
  counts10[8] = (long)w[PO_W_DRY];
  counts10[9] = (long)w[PO_W_SKIPPED];
  V.ncomp = ncomp;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_pore_labels(lbmdem_handle* h, int* label) try {
  CHECK_H(h);
  if (!label) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(pores_ready(h, "lbmdem_download_pore_labels"));
  RC_TRY(stage_download_plane(h, label, h->po.label));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_pore_labels_device(lbmdem_handle* h, const int** label, int* sy) try {
  CHECK_H(h);
  if (!label || !sy) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(pores_ready(h, "lbmdem_pore_labels_device"));
  *label = h->po.label;
  *sy = h->L.sy;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_pores(lbmdem_handle* h, lbmdem_pore* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(pores_ready(h, "lbmdem_download_pores"));
  return stage_table(h, "lbmdem_download_pores", "components", h->po.table, sizeof *out, h->po.ncomp, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_pore_grains(lbmdem_handle* h, int* wet, int* pore_min, int* pore_max) try {
  CHECK_H(h);
  RC_TRY(pores_ready(h, "lbmdem_download_pore_grains"));
  const size_t n = (size_t)h->n;
  int* const g[3] = {wet, pore_min, pore_max};
  for (int k = 0; k < 3; ++k)
    if (g[k]) HIP_TRY(hipMemcpyAsync(g[k], h->po.grains + k * n, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_pore_grains_device(lbmdem_handle* h, const int** wet, const int** pore_min, const int** pore_max) try {
  CHECK_H(h);
  RC_TRY(pores_ready(h, "lbmdem_pore_grains_device"));
  const size_t n = (size_t)h->n;
  const int** const g[3] = {wet, pore_min, pore_max};
  for (int k = 0; k < 3; ++k)
    if (g[k]) *g[k] = h->po.grains + k * n;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_pores(lbmdem_handle* h, const char* dir, int nfile, int conn, int plane) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_pores"));
  const LatticeView& L = h->L;
  const size_t n = (size_t)h->n;
  long counts[LBMDEM_PORE_COUNTS], ntable = 0;
  RC_TRY(lbmdem_pore_compute(h, conn, nullptr, counts));
  RC_TRY(lbmdem_download_pores(h, nullptr, 0, &ntable));
  std::vector<lbmdem_pore> table((size_t)ntable);
  if (ntable > 0) RC_TRY(lbmdem_download_pores(h, table.data(), ntable, &ntable));
  std::vector<int> g(3 * n), label;
  RC_TRY(lbmdem_download_pore_grains(h, g.data(), g.data() + n, g.data() + 2 * n));
  if (plane) {
    label.resize((size_t)L.lx * L.ly);
    RC_TRY(lbmdem_download_pore_labels(h, label.data()));
  }
  return lbmdem_write_pore_files(dir, nfile, conn, L.lx, L.ly, plane, plane ? label.data() : nullptr, ntable > 0 ? table.data() : nullptr,
                                 ntable, (int)n, g.data(), g.data() + n, g.data() + 2 * n, counts, h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_pores_output(lbmdem_handle* h, int on, int conn, int plane) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_pores_output"));
    if (conn != 4 && conn != 8) return fail(LBMDEM_EINVAL, "lbmdem_set_pores_output: conn is 4 or 8 (%d)", conn);
    h->pores_conn = conn;
    h->pores_plane = plane != 0;
  }
  h->pores_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
