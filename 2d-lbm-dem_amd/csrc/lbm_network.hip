// lbm_network.hip -- the pore network: a watershed of the clearance analysis' exact squared distance d2. Every fluid node climbs to
// the local maximum of d2 it belongs to (the pore bodies), the highest pass between two adjacent basins is their link's saddle,
// bodies separated by a pass almost as high as the lower summit merge into one group, and the same links are made again between
// the groups (lbmdem_network_compute, lbmdem_download_network, lbmdem_network_device, lbmdem_download_network_bodies,
// lbmdem_download_network_groups, lbmdem_download_network_links, lbmdem_write_network, lbmdem_set_network_output,
// lbmdem_write_network_files; include/lbmdem_hip.h, "Pore network", has the contract in full). Every result is an integer and
// every tie has a rule, so nothing depends on the order anything happens in. Nothing here is on the step path: the kernels read
// the ClearanceStage's d2 and write to the handle's NetworkStage, and nothing is allocated or launched before the first compute.
//
// "Higher" is the order of the packed key d2 << 32 | (lx*ly - 1 - k), k = x*ly + y the host index. In the device layout
// (node = x*sy + y, which orders the nodes as k does), on the handle's stream:
//   k_nw_ascent   a tile of 16 x 64 nodes with a one-node apron of keys in LDS, lanes along y: a node takes the highest of itself
//                 and its 8 neighbours; the chains inside the tile are shortened by pointer jumping in LDS until every node points
//                 at a peak of the tile or at the node outside the tile its chain leaves through;
//   k_nw_find     a node follows these pointers across tiles, strictly upward, to its peak. It may write any ancestor over a
//                 pointer another lane is reading: every value a pointer ever holds is a higher node of the same basin;
//   k_nw_peaks, a scan, k_nw_number   the peaks numbered in node order: the bodies;
//   k_nw_label    the body plane, and the nodes per body (the lanes of a wavefront that share a body first, an LDS slot per body
//                 modulo 64, then 64-bit atomics);
//   k_nw_count, a scan, k_nw_emit   per pair of 8-adjacent fluid nodes with different labels one record
//                 (lo * B + hi, (dtop - height) << pbits | node);
//   two stable hipcub::DeviceRadixSort passes, by value and then by pair, a run-length encode and a scan of the run lengths;
//   k_nw_links    one record per run: its pair, its length, and from its first record the largest height and that one's
//                 smallest node; the two bodies' degrees;
//   k_nw_propose, k_nw_parent, k_nw_root   the merge: a link proposes the higher body to the lower one by an atomic maximum of
//                 saddle << 32 | ~partner -- the maximum IS rule 4's choice, so the order of the proposals does not matter --, then
//                 every body follows the parents to its root;
//   k_nw_group    the group plane; the count / sort / encode stage runs again over it;
//   k_nw_flag, a scan, k_nw_groups, k_nw_gather, k_nw_census   the group records and the counts.
// Single launches, no host-driven rounds, no workgroup waits for another, integer atomics only, no floating point anywhere. Every
// loop has the bound its comment states.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both. Front end, as every export's: whole_handle(), SP_REFUSE() (lbmdem_handle.h), MemPool (lbm_mem.h) for what is kept on the
// handle and for a call's sort records, OutFile (lbm_outfile.h) for the files; what the pore stages share, lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

constexpr int NW_SIDE_MAX = 32768;   // the clearance analysis': d2 < 2^31, a node's index < 2^30

#ifndef LBMDEM_SINGLE_PRECISION
typedef unsigned long long nw_u64;
constexpr int NW_THREADS = 256;
constexpr int NW_TX = 16, NW_TY = 64;   // the ascent's tile: rows x columns
constexpr int NW_SLOTS = 64;            // LDS slots of the bodies' node counts, by body modulo NW_SLOTS
// NetworkStage::words
enum : int { NW_W_FLUID = 0, NW_W_ISOLATED, NW_W_LARGEST, NW_W_NARROWEST, NW_WORDS };

struct NwJob {
  const int* d2;     // [lx][sy] the clearance analysis' plane: > 0 exactly on the fluid, 0 in the pad columns
  int lx, ly, sy;
  long N, Nh;        // lx * sy, lx * ly
  int* par;          // [lx][sy]
  int* body;         // [lx][sy]
  int* group;        // [lx][sy]
  nw_u64* words;
  nw_u64* cnt;       // [nblocks + 1] per block of NW_THREADS nodes
  nw_u64* off;       // [nblocks + 1] their scan
  long nblocks;
  lbmdem_net_body* bodies;
  long B;
  int* grp;          // [B] a higher body of the same group, in the end the root
  int* deg;          // [B] the degrees of the level at work
  int* flag;         // [B + 1] 1 at the roots
  int* gi;           // [B + 1] the scan: a root's place in the group table
  nw_u64* best;      // [B]
  int merge;
  const int* lab;    // the label plane of the level at work: body or group
  nw_u64* rk;        // [nedges] pair keys, lo * B + hi
  nw_u64* rv;        // [nedges] (dtop - height) << pbits | p
  long nedges;
  int pbits;         // bits of a host index
  long dtop;         // above every d2
  const nw_u64* uniq;   // [nlinks] the pair keys, ascending
  const int* runs;      // [nlinks] their run lengths
  const int* offs;      // [nlinks] the runs' first records
  lbmdem_net_link* table;
  long nlinks;
  lbmdem_net_group* groups;
  long G;
};

__device__ __forceinline__ int nw_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The tile's keys with a one-node apron; 0 where there is no fluid node (a fluid node's key has d2 >= 1).
__global__ __launch_bounds__(NW_THREADS) void k_nw_ascent(const NwJob J) {
  __shared__ nw_u64 s_key[NW_TX + 2][NW_TY + 2];
  __shared__ int s_up[NW_TX * NW_TY];   // >= 0: a node of the tile; -1: not fluid; <= -2: the device node -2 - value outside the tile
  const int x0 = blockIdx.y * NW_TX, y0 = blockIdx.x * NW_TY;
  for (int i = threadIdx.x; i < (NW_TX + 2) * (NW_TY + 2); i += NW_THREADS) {
    const int r = i / (NW_TY + 2), c = i % (NW_TY + 2);
    const int x = x0 - 1 + r, y = y0 - 1 + c;
    nw_u64 k = 0;
    if (x >= 0 && x < J.lx && y >= 0 && y < J.ly) {
      const int d = J.d2[(long)x * J.sy + y];
      if (d > 0) k = (nw_u64)(unsigned)d << 32 | (nw_u64)(unsigned)(J.Nh - 1 - ((long)x * J.ly + y));
    }
    s_key[r][c] = k;
  }
  __syncthreads();
  const int c = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < NW_TX; r += NW_THREADS / 64) {
    const nw_u64 me = s_key[r + 1][c + 1];
    int v = -1;
    if (me) {
      nw_u64 top = me;
      int br = 0, bc = 0;
#pragma unroll
      for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) {
          const nw_u64 o = s_key[r + 1 + dr][c + 1 + dc];
          if (o > top) { top = o; br = dr; bc = dc; }   // (the keys of fluid nodes differ)
        }
      const int tr = r + br, tc = c + bc;
      if (tr >= 0 && tr < NW_TX && tc >= 0 && tc < NW_TY) v = tr * NW_TY + tc;
      else v = -2 - (int)((long)(x0 + tr) * J.sy + (y0 + tc));   // (a fluid node: inside the lattice)
    }
    s_up[r * NW_TY + c] = v;
  }
  __syncthreads();
  // Pointer jumping: a node whose target is a node of the tile that is not a peak takes that node's target. A target is only ever
  // replaced by a higher node of the same chain, so a round that reads a value another lane is replacing reads an ancestor either
  // way. A chain of the tile has fewer than NW_TX * NW_TY steps and every round with a change shortens one: at most that many rounds,
  // about log2 of the longest chain in practice.
  for (int round = 0; round < NW_TX * NW_TY; ++round) {
    int changed = 0;
    for (int r = threadIdx.x >> 6; r < NW_TX; r += NW_THREADS / 64) {
      const int li = r * NW_TY + c;
      const int v = s_up[li];
      if (v >= 0 && v != li) {
        const int w = s_up[v];
        if (w != v) { s_up[li] = w; changed = 1; }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  for (int r = threadIdx.x >> 6; r < NW_TX; r += NW_THREADS / 64) {
    const int x = x0 + r, y = y0 + c;
    if (x >= J.lx || y >= J.sy) continue;
    const int v = s_up[r * NW_TY + c];
    J.par[(long)x * J.sy + y] = v >= 0 ? (int)((long)(x0 + v / NW_TY) * J.sy + (y0 + v % NW_TY)) : v == -1 ? -1 : -2 - v;
  }
}

// Across the tiles: every step goes to a higher node, so the walk ends at the peak within the basin's longest chain of tile exits
// (fewer than N steps). The store may race with the walks of other lanes through this node: they read the old or the new value,
// and both are ancestors.
__global__ __launch_bounds__(NW_THREADS) void k_nw_find(const NwJob J) {
  const long node = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (node >= J.N) return;
  const int p = nw_load(J.par + node);
  if (p < 0) return;
  int r = p;
  for (long step = 0; step < J.N; ++step) {
    const int q = nw_load(J.par + r);
    if (q == r || q < 0 || q >= J.N) break;   // (q == r: the peak; the rest never happens)
    r = q;
  }
  if (r != p) J.par[node] = r;
}

__device__ __forceinline__ nw_u64 nw_wave_sum(nw_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}

// cnt[block] from one number per thread
__device__ __forceinline__ void nw_block_count(const NwJob& J, int mine) {
  __shared__ nw_u64 part[NW_THREADS / 64];
  const nw_u64 w = nw_wave_sum((nw_u64)mine);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    nw_u64 s = 0;
    for (int k = 0; k < NW_THREADS / 64; ++k) s += part[k];
    J.cnt[blockIdx.x] = s;
    if (blockIdx.x == 0) J.cnt[J.nblocks] = 0;   // the scan's last item
  }
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_peaks(const NwJob J) {
  const long node = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  nw_block_count(J, node < J.N && J.par[node] == (int)node);
}

// The peaks' numbers go to the group plane at the peaks: k_nw_group overwrites the plane later.
__global__ __launch_bounds__(NW_THREADS) void k_nw_number(const NwJob J) {
  typedef hipcub::BlockScan<int, NW_THREADS> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const long node = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  const int mine = node < J.N && J.par[node] == (int)node;
  int before = 0;
  Scan(tmp).ExclusiveSum(mine, before);
  const long b = (long)J.off[blockIdx.x] + before;
  if (mine && b < J.B) {   // (always: B is the scan's total)
    J.group[node] = (int)b;
    lbmdem_net_body e;
    e.node = (int)((node / J.sy) * J.ly + node % J.sy);
    e.d2 = J.d2[node];
    e.nodes = 0;
    e.degree = 0;
    e.parent = (int)b;
    e.group = (int)b;
    J.bodies[b] = e;
  }
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_label(const NwJob J) {
  __shared__ int s_lab[NW_SLOTS];
  __shared__ nw_u64 s_cnt[NW_SLOTS];
  if (threadIdx.x < NW_SLOTS) { s_lab[threadIdx.x] = -1; s_cnt[threadIdx.x] = 0; }
  __syncthreads();
  const long node = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int b = -1;
  if (node < J.N) {
    const int p = J.par[node];
    if (p >= 0 && p < J.N) b = J.group[p];   // (a peak's number)
    if (b < 0 || b >= J.B) b = -1;           // (never)
    J.body[node] = b;
  }
  // the lanes that share a body: every round retires its leader's lanes, 64 rounds at most
  nw_u64 todo = __ballot(b >= 0);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int bb = __shfl(b, lead);
    const nw_u64 same = __ballot(b == bb);
    if (lane == lead) {
      const int slot = bb & (NW_SLOTS - 1);
      const int held = atomicCAS(&s_lab[slot], -1, bb);
      if (held == -1 || held == bb) atomicAdd(&s_cnt[slot], (nw_u64)__popcll(same));
      else atomicAdd(reinterpret_cast<nw_u64*>(&J.bodies[bb].nodes), (nw_u64)__popcll(same));
    }
    todo &= ~same;
  }
  __syncthreads();
  if (threadIdx.x < NW_SLOTS && s_lab[threadIdx.x] >= 0)
    atomicAdd(reinterpret_cast<nw_u64*>(&J.bodies[s_lab[threadIdx.x]].nodes), s_cnt[threadIdx.x]);
}

// The edges that start at a device node p, towards the nodes q > p adjacent to it: (x, y + 1), (x + 1, y - 1), (x + 1, y),
// (x + 1, y + 1). A label is >= 0 exactly on the fluid; the pad columns hold -1.
__device__ __forceinline__ int nw_edges_of(const NwJob& J, long node, nw_u64* rk, nw_u64* rv) {
  if (node >= J.N) return 0;
  const int x = (int)(node / J.sy), y = (int)(node % J.sy);
  if (y >= J.ly) return 0;
  const int l = J.lab[node];
  if (l < 0) return 0;
  const int d = J.d2[node];
  const nw_u64 p = (nw_u64)((long)x * J.ly + y);
  int cnt = 0;
  const int dxs[4] = {0, 1, 1, 1}, dys[4] = {1, -1, 0, 1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xq = x + dxs[k], yq = y + dys[k];
    if (xq >= J.lx || yq < 0 || yq >= J.ly) continue;
    const long q = node + (long)dxs[k] * J.sy + dys[k];
    const int l1 = J.lab[q];
    if (l1 < 0 || l1 == l) continue;
    const int d1 = J.d2[q];
    const int lo = l < l1 ? l : l1, hi = l < l1 ? l1 : l;
    rk[cnt] = (nw_u64)lo * (nw_u64)J.B + (nw_u64)hi;
    rv[cnt] = (nw_u64)(J.dtop - (d < d1 ? d : d1)) << J.pbits | p;   // the largest height first, then the smallest p
    ++cnt;
  }
  return cnt;
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_count(const NwJob J) {
  nw_u64 rk[4], rv[4];
  nw_block_count(J, nw_edges_of(J, (long)blockIdx.x * NW_THREADS + threadIdx.x, rk, rv));
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_emit(const NwJob J) {
  typedef hipcub::BlockScan<int, NW_THREADS> Scan;
  __shared__ typename Scan::TempStorage tmp;
  nw_u64 rk[4], rv[4];
  const int mine = nw_edges_of(J, (long)blockIdx.x * NW_THREADS + threadIdx.x, rk, rv);
  int before = 0;
  Scan(tmp).ExclusiveSum(mine, before);
  const long at = (long)J.off[blockIdx.x] + before;
  for (int k = 0; k < mine; ++k)
    if (at + k < J.nedges) {   // (always: nedges is the scan's total)
      J.rk[at + k] = rk[k];
      J.rv[at + k] = rv[k];
    }
}

// One link per run of equal pairs; the records of a run ascend by (dtop - height, node).
__global__ __launch_bounds__(NW_THREADS) void k_nw_links(const NwJob J) {
  const long t = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (t >= J.nlinks) return;
  const nw_u64 key = J.uniq[t];
  const long first = J.offs[t];
  const nw_u64 v = first >= 0 && first < J.nedges ? J.rv[first] : 0ull;   // (always inside)
  lbmdem_net_link e;
  e.lo = (int)(key / (nw_u64)J.B);
  e.hi = (int)(key % (nw_u64)J.B);
  e.edges = J.runs[t];
  e.saddle = (int)(J.dtop - (long)(v >> J.pbits));
  e.node = (int)(v & ((1ull << J.pbits) - 1ull));
  J.table[t] = e;
  if (e.lo >= 0 && e.hi < J.B) {   // (always)
    atomicAdd(&J.deg[e.lo], 1);
    atomicAdd(&J.deg[e.hi], 1);
  }
}

// floor(sqrt(v)) in integers, 16 rounds
__device__ __forceinline__ int nw_isqrt(unsigned v) {
  unsigned r = 0;
#pragma unroll
  for (unsigned b = 1u << 15; b; b >>= 1) {
    const unsigned t = r | b;
    if (t * t <= v) r = t;
  }
  return (int)r;
}

// A level-0 link proposes its higher body b to its lower body a when the pass is high enough. Bodies are numbered in node order,
// so among equal d2 the smaller number is the higher peak. (A saddle is >= 1: 0 says "no candidate".)
__global__ __launch_bounds__(NW_THREADS) void k_nw_propose(const NwJob J) {
  const long t = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (t >= J.nlinks) return;
  const lbmdem_net_link e = J.table[t];
  if (e.lo < 0 || e.hi >= J.B) return;   // (never)
  const int dlo = J.bodies[e.lo].d2, dhi = J.bodies[e.hi].d2;
  const int a = dlo >= dhi ? e.hi : e.lo, b = dlo >= dhi ? e.lo : e.hi;   // (lo < hi: equal d2 makes lo the higher)
  const int da = dlo >= dhi ? dhi : dlo;
  if (nw_isqrt((unsigned)da) - nw_isqrt((unsigned)e.saddle) <= J.merge)
    atomicMax(&J.best[a], (nw_u64)(unsigned)e.saddle << 32 | (nw_u64)(0xFFFFFFFFu - (unsigned)b));
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_parent(const NwJob J) {
  const long a = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (a >= J.B) return;
  const nw_u64 w = J.best[a];
  int b = w ? (int)(0xFFFFFFFFu - (unsigned)w) : (int)a;
  if (b < 0 || b >= J.B) b = (int)a;   // (never)
  J.bodies[a].parent = b;
  J.bodies[a].degree = J.deg[a];
  J.grp[a] = b;
}

// k_nw_find's walk over the bodies: a parent is a higher body, fewer than B steps
__global__ __launch_bounds__(NW_THREADS) void k_nw_root(const NwJob J) {
  const long a = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (a >= J.B) return;
  const int p = nw_load(J.grp + a);
  int r = p;
  for (long step = 0; step < J.B; ++step) {
    const int q = nw_load(J.grp + r);
    if (q == r) break;
    r = q;
  }
  if (r != p) J.grp[a] = r;
  J.bodies[a].group = r;
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_group(const NwJob J) {
  const long node = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (node >= J.N) return;
  const int b = J.body[node];
  J.group[node] = b >= 0 ? J.grp[b] : -1;
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_flag(const NwJob J) {
  const long a = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (a <= J.B) J.flag[a] = a < J.B && J.grp[a] == (int)a;
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_groups(const NwJob J) {
  const long a = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (a >= J.B || !J.flag[a]) return;
  const int g = J.gi[a];
  if (g < 0 || g >= J.G) return;   // (never)
  const lbmdem_net_body e = J.bodies[a];
  lbmdem_net_group o;
  o.body = (int)a;
  o.bodies = 0;
  o.nodes = 0;
  o.d2 = e.d2;
  o.node = e.node;
  o.degree = J.deg[a];
  J.groups[g] = o;
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_gather(const NwJob J) {
  const long a = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  if (a >= J.B) return;
  const int g = J.gi[J.grp[a]];
  if (g < 0 || g >= J.G) return;   // (never)
  atomicAdd(&J.groups[g].bodies, 1);
  atomicAdd(reinterpret_cast<nw_u64*>(&J.groups[g].nodes), (nw_u64)J.bodies[a].nodes);
}

__global__ __launch_bounds__(NW_THREADS) void k_nw_census(const NwJob J) {
  const long i = (long)blockIdx.x * NW_THREADS + threadIdx.x;
  nw_u64 nodes = 0, top = 0, low = ~0ull;
  bool alone = false;
  if (i < J.G) {
    const lbmdem_net_group e = J.groups[i];
    nodes = top = (nw_u64)e.nodes;
    alone = e.degree == 0;
  }
  if (i < J.nlinks) low = (nw_u64)(unsigned)J.table[i].saddle;
  nodes = nw_wave_sum(nodes);
  for (int m = 32; m >= 1; m >>= 1) {
    const nw_u64 o = __shfl_xor(top, m), u = __shfl_xor(low, m);
    top = o > top ? o : top;
    low = u < low ? u : low;
  }
  const nw_u64 nalone = __popcll(__ballot(alone));
  if ((threadIdx.x & 63) == 0) {
    if (nodes) { atomicAdd(&J.words[NW_W_FLUID], nodes); atomicMax(&J.words[NW_W_LARGEST], top); }
    if (nalone) atomicAdd(&J.words[NW_W_ISOLATED], nalone);
    if (low != ~0ull) atomicMin(&J.words[NW_W_NARROWEST], low);
  }
}

// what depends on the lattice, once
int network_stage(lbmdem_handle* h) {
  auto& V = h->net;
  if (V.words) return LBMDEM_OK;
  const size_t N = (size_t)h->L.lx * h->L.sy;
  const long nb = stage_blocks((long)N, NW_THREADS);
  HIP_TRY(h->mem.dev(&V.par, N));
  HIP_TRY(h->mem.dev(&V.body, N));
  HIP_TRY(h->mem.dev(&V.group, N));
  HIP_TRY(h->mem.dev(&V.cnt, 2 * ((size_t)nb + 1)));
  HIP_TRY(h->mem.dev(&V.nruns, (size_t)1));
  HIP_TRY(h->mem.dev(&V.words, (size_t)NW_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

int network_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  if (!h->net.at.current(h))
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_network_compute has been made for the map as it is now", who);
  return LBMDEM_OK;
}

// The links of one level: J.lab is the label plane, J.deg the degrees (zeroed). Count, scan, emit, sort, encode, table. The sort's
// records are this call's alone (40 bytes an edge): a pool of its own, gone at the return. -> *nedges, *nlinks, V.links[level]
int network_links(lbmdem_handle* h, NwJob& J, int level, long max_edges, long* nedges, long* nlinks) {
  auto& V = h->net;
  const hipStream_t st = h->stream;
  MemPool scratch;
  hipLaunchKernelGGL(k_nw_count, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  char* tmp = nullptr;
  size_t b = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, J.cnt, J.off, (int)(J.nblocks + 1), st));
  HIP_TRY(scratch.dev(&tmp, b));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, b, J.cnt, J.off, (int)(J.nblocks + 1), st));
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, J.off + J.nblocks, sizeof total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (total > (unsigned long long)(max_edges > 0 ? max_edges : (long)INT_MAX))
    return fail(LBMDEM_EINVAL, "lbmdem_network_compute: the ridge has %llu edges, max_edges is %ld", total,
                max_edges > 0 ? max_edges : (long)INT_MAX);
  const int E = (int)total;
  int T = 0;
  J.nedges = E;
  if (E > 0) {
    nw_u64 *rk0 = nullptr, *rk1 = nullptr, *rv0 = nullptr, *rv1 = nullptr, *uniq = nullptr;
    int *runs = nullptr, *offs = nullptr;
    HIP_TRY(scratch.dev(&rk0, (size_t)E)); HIP_TRY(scratch.dev(&rk1, (size_t)E));
    HIP_TRY(scratch.dev(&rv0, (size_t)E)); HIP_TRY(scratch.dev(&rv1, (size_t)E));
    HIP_TRY(scratch.dev(&uniq, (size_t)E));
    HIP_TRY(scratch.dev(&runs, (size_t)E)); HIP_TRY(scratch.dev(&offs, (size_t)E));
    J.rk = rk0; J.rv = rv0;
    hipLaunchKernelGGL(k_nw_emit, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    const int vbits = J.pbits + stage_bits((unsigned long long)J.dtop);
    const int kbits = stage_bits((unsigned long long)J.B * (unsigned long long)J.B);
    size_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, rv0, rv1, rk0, rk1, E, 0, vbits, st));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b2, rk1, rk0, rv1, rv0, E, 0, kbits, st));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, b3, rk0, uniq, runs, V.nruns, E, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b4, runs, offs, E, st));
    b = b1 > b2 ? b1 : b2; b = b > b3 ? b : b3; b = b > b4 ? b : b4;
    char* big = nullptr;
    HIP_TRY(scratch.dev(&big, b));
    size_t bb = b;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(big, bb, rv0, rv1, rk0, rk1, E, 0, vbits, st));   // by (height descending, node)
    bb = b;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(big, bb, rk1, rk0, rv1, rv0, E, 0, kbits, st));   // stable: then by pair
    bb = b;
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(big, bb, rk0, uniq, runs, V.nruns, E, st));
    HIP_TRY(hipMemcpyAsync(&T, V.nruns, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bb = b;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(big, bb, runs, offs, T, st));
    HIP_TRY(h->mem.grow(&V.links[level], &V.link_cap[level], (long)T + T / 4 + 64));
    J.uniq = uniq; J.runs = runs; J.offs = offs;
    J.table = V.links[level]; J.nlinks = T;
    hipLaunchKernelGGL(k_nw_links, dim3((unsigned)stage_blocks(T, NW_THREADS)), dim3(NW_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the records go with `scratch`)
  }
  J.table = V.links[level]; J.nlinks = T;
  *nedges = E; *nlinks = T;
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_network_files(const char* dir, int nfile, int lx, int ly, int n, int merge, int plane, const int* body,
                               const int* group, const lbmdem_net_body* bodies, long nbodies, const lbmdem_net_group* groups,
                               long ngroups, const lbmdem_net_link* links, long nlinks, const long* counts10, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || merge < -1 || nbodies < 0 || ngroups < 0 || nlinks < 0 || (nbodies > 0 && !bodies) || (ngroups > 0 && !groups) ||
      (nlinks > 0 && !links) || !counts10 || (plane && (!body || !group)))
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_network_files arguments");
  if (lx < 2 || ly < 2 || lx > NW_SIDE_MAX || ly > NW_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: the lattice is %d x %d", lx, ly);
  const long cnt = (long)lx * ly;
  for (long k = 0; k < nbodies; ++k) {
    const lbmdem_net_body& e = bodies[k];
    if (e.d2 < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: body %ld has the negative d2 %d", k, e.d2);
    if (e.node < 0 || e.node >= cnt || (k > 0 && e.node <= bodies[k - 1].node))
      return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: body %ld has the node %d: the nodes ascend, 0 <= node < %ld", k, e.node, cnt);
    if (e.group < 0 || e.group >= nbodies || bodies[e.group].group != e.group)
      return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: body %ld has the group %d, which is not a root", k, e.group);
  }
  for (long k = 0; k < ngroups; ++k) {
    const lbmdem_net_group& e = groups[k];
    if (e.d2 < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: group %ld has the negative d2 %d", k, e.d2);
    if (e.body < 0 || e.body >= nbodies || (k > 0 && e.body <= groups[k - 1].body))
      return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: group %ld has the body %d: the bodies ascend, 0 <= body < %ld", k, e.body, nbodies);
    if (bodies[e.body].group != e.body)
      return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: group %ld has the body %d, which is not a root", k, e.body);
  }
  for (long k = 0; k < nlinks; ++k) {
    const lbmdem_net_link& e = links[k];
    const bool ascends = k == 0 || e.lo > links[k - 1].lo || (e.lo == links[k - 1].lo && e.hi > links[k - 1].hi);
    if (e.lo < 0 || e.lo >= e.hi || e.hi >= nbodies || !ascends)
      return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: link %ld has the pair (%d, %d): the pairs ascend, 0 <= lo < hi < %ld",
                  k, e.lo, e.hi, nbodies);
    if (bodies[e.lo].group != e.lo || bodies[e.hi].group != e.hi)
      return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: link %ld joins (%d, %d), which are not both roots", k, e.lo, e.hi);
  }
  if (plane)
    for (long k = 0; k < cnt; ++k)
      if (body[k] < -1 || body[k] >= nbodies || group[k] < -1 || group[k] >= nbodies)
        return fail(LBMDEM_EINVAL, "lbmdem_write_network_files: body[%ld][%ld] = %d, group = %d: -1 or a body's number below %ld",
                    k / ly, k % ly, body[k], group[k], nbodies);
  OutFile F;
  RC_TRY(F.open("w", dir, "network_bodies%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d\n", lx, ly, n, merge);
  fprintf(fp, "# body node d2 nodes degree parent group\n");
  for (long k = 0; k < nbodies; ++k) {
    const lbmdem_net_body& e = bodies[k];
    fprintf(fp, "%ld %d %d %ld %d %d %d\n", k, e.node, e.d2, e.nodes, e.degree, e.parent, e.group);
  }
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "network_links%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d\n", lx, ly, n, merge);
  fprintf(fp, "# lo hi edges saddle node\n");
  for (long k = 0; k < nlinks; ++k) {
    const lbmdem_net_link& e = links[k];
    fprintf(fp, "%d %d %d %d %d\n", e.lo, e.hi, e.edges, e.saddle, e.node);
  }
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "network_groups%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d merge %d\n", lx, ly, n, merge);
  fprintf(fp, "# body bodies nodes d2 node degree\n");
  for (long k = 0; k < ngroups; ++k) {
    const lbmdem_net_group& e = groups[k];
    fprintf(fp, "%d %d %ld %d %d %d\n", e.body, e.bodies, e.nodes, e.d2, e.node, e.degree);
  }
  RC_TRY(F.close());
  if (plane) {
    const int* const planes[2] = {body, group};
    const char* const names[2] = {"body", "group"};
    RC_TRY(stage_write_int_planes(F, dir, nfile, "network%.6i.vtk", "lbmdem pore network", lx, ly, names, planes, 2));
  }
  return stage_append_row(F, dir, "network.data",
                          "# t fluid_nodes bodies body_links body_edges groups group_links group_edges isolated_groups "
                          "largest_group_nodes narrowest_saddle", t, counts10, LBMDEM_NETWORK_COUNTS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_network_compute(lbmdem_handle* h, const int*, int, long, long*) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_download_network(lbmdem_handle* h, int*, int*) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_network_device(lbmdem_handle* h, const int**, const int**, int*) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_download_network_bodies(lbmdem_handle* h, lbmdem_net_body*, long, long*) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_download_network_groups(lbmdem_handle* h, lbmdem_net_group*, long, long*) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_download_network_links(lbmdem_handle* h, int, lbmdem_net_link*, long, long*) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_write_network(lbmdem_handle* h, const char*, int, int, int) { SP_REFUSE(h, "the pore network analysis"); }
int lbmdem_set_network_output(lbmdem_handle* h, int, int, int) { SP_REFUSE(h, "the pore network analysis"); }
#else

int lbmdem_network_compute(lbmdem_handle* h, const int* map, int merge, long max_edges, long* counts10) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_network_compute"));
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  if (lx > NW_SIDE_MAX || ly > NW_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_network_compute: a lattice of %d x %d nodes has a side above %d: the squared distances are "
                               "32-bit integers", lx, ly, NW_SIDE_MAX);
  if (merge < -1) return fail(LBMDEM_EINVAL, "lbmdem_network_compute: merge must be -1 (no merging) or a difference of radii >= 0 (%d)", merge);
  RC_TRY(stage_check_max_edges("lbmdem_network_compute", max_edges));
  auto& V = h->net;
  V.at.valid = false;
  ++V.gen;
  RC_TRY(stage_check_map("lbmdem_network_compute", map, lx, ly, n));
  // the clearance first: its d2 of the handle's map is reused while its guard calls it valid
  const auto& Q = h->clr;
  if (map || !(Q.at.current(h) && Q.own)) {
    long cc[LBMDEM_CLEARANCE_COUNTS];
    RC_TRY(lbmdem_clearance_compute(h, map, 0, cc));
  }
  RC_TRY(network_stage(h));
  const hipStream_t st = h->stream;
  const long N = (long)lx * sy;
  NwJob J{};
  J.d2 = Q.d2;
  J.lx = lx; J.ly = ly; J.sy = sy;
  J.N = N; J.Nh = (long)lx * ly;
  J.par = V.par; J.body = V.body; J.group = V.group;
  J.words = V.words;
  J.nblocks = stage_blocks(N, NW_THREADS);
  J.cnt = V.cnt; J.off = V.cnt + J.nblocks + 1;
  J.merge = merge;
  J.pbits = stage_bits((unsigned long long)(J.Nh - 1));
  const int side = lx < ly ? lx : ly;
  J.dtop = (long)((side + 1) / 2 + 1) * ((side + 1) / 2 + 1);
  HIP_TRY(hipMemsetAsync(V.words, 0, sizeof(nw_u64) * NW_WORDS, st));
  HIP_TRY(hipMemsetAsync(V.words + NW_W_NARROWEST, 0xFF, sizeof(nw_u64), st));   // (a minimum)
  hipLaunchKernelGGL(k_nw_ascent, dim3((unsigned)stage_blocks(sy, NW_TY), (unsigned)stage_blocks(lx, NW_TX)), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_find, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_peaks, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  long B = 0;
  {
    MemPool scratch;
    char* tmp = nullptr;
    size_t b = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, J.cnt, J.off, (int)(J.nblocks + 1), st));
    HIP_TRY(scratch.dev(&tmp, b));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, b, J.cnt, J.off, (int)(J.nblocks + 1), st));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, J.off + J.nblocks, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    B = (long)total;   // (<= lx * ly < 2^31)
  }
  if (V.body_cap < B + 1) {   // the per-body blocks go and come together; body_cap says so only once all three are there
    const long want = B + B / 4 + 64;
    V.body_cap = 0;
    h->mem.release(V.bodies); V.bodies = nullptr;
    h->mem.release(V.barr); V.barr = nullptr;
    h->mem.release(V.best); V.best = nullptr;
    HIP_TRY(h->mem.dev(&V.bodies, (size_t)want));
    HIP_TRY(h->mem.dev(&V.barr, 5 * ((size_t)want + 1)));
    HIP_TRY(h->mem.dev(&V.best, (size_t)want));
    V.body_cap = want;
  }
  const long cap1 = V.body_cap + 1;
  int* const deg0 = V.barr + cap1;
  int* const deg1 = V.barr + 2 * cap1;
  J.bodies = V.bodies; J.B = B;
  J.grp = V.barr; J.flag = V.barr + 3 * cap1; J.gi = V.barr + 4 * cap1;
  J.best = V.best;
  HIP_TRY(hipMemsetAsync(deg0, 0, sizeof(int) * 2 * (size_t)cap1, st));   // both levels' degrees
  HIP_TRY(hipMemsetAsync(V.best, 0, sizeof(nw_u64) * (size_t)(B > 0 ? B : 1), st));
  hipLaunchKernelGGL(k_nw_number, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_label, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  long E0 = 0, L0 = 0, E1 = 0, L1 = 0, G = 0;
  const unsigned bblocks = (unsigned)stage_blocks(B + 1, NW_THREADS);
  J.lab = V.body; J.deg = deg0;
  RC_TRY(network_links(h, J, 0, max_edges, &E0, &L0));
  if (merge >= 0 && L0 > 0) hipLaunchKernelGGL(k_nw_propose, dim3((unsigned)stage_blocks(L0, NW_THREADS)), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_parent, dim3(bblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_root, dim3(bblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_group, dim3((unsigned)J.nblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_flag, dim3(bblocks), dim3(NW_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  {
    MemPool scratch;
    char* tmp = nullptr;
    size_t b = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, J.flag, J.gi, (int)(B + 1), st));
    HIP_TRY(scratch.dev(&tmp, b));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, b, J.flag, J.gi, (int)(B + 1), st));
    int total = 0;
    HIP_TRY(hipMemcpyAsync(&total, J.gi + B, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    G = total;
  }
  J.lab = V.group; J.deg = deg1;
  RC_TRY(network_links(h, J, 1, 0, &E1, &L1));
  HIP_TRY(h->mem.grow(&V.groups, &V.group_cap, G + G / 4 + 64));
  J.groups = V.groups; J.G = G;
  hipLaunchKernelGGL(k_nw_groups, dim3(bblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_gather, dim3(bblocks), dim3(NW_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_nw_census, dim3((unsigned)stage_blocks((G > L1 ? G : L1) + 1, NW_THREADS)), dim3(NW_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[NW_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts10[0] = (long)w[NW_W_FLUID];
  counts10[1] = B;
  counts10[2] = L0;
  counts10[3] = E0;
  counts10[4] = G;
  counts10[5] = L1;
  counts10[6] = E1;
  counts10[7] = (long)w[NW_W_ISOLATED];
  counts10[8] = (long)w[NW_W_LARGEST];
  counts10[9] = L1 > 0 ? (long)w[NW_W_NARROWEST] : -1;
  V.nbodies = B; V.ngroups = G; V.nlinks[0] = L0; V.nlinks[1] = L1;
  V.own = map == nullptr;
  V.merge = merge;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_network(lbmdem_handle* h, int* body, int* group) try {
  CHECK_H(h);
  if (!body && !group) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(network_ready(h, "lbmdem_download_network"));
  if (body) RC_TRY(stage_download_plane(h, body, h->net.body));
  if (group) RC_TRY(stage_download_plane(h, group, h->net.group));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_network_device(lbmdem_handle* h, const int** body, const int** group, int* sy) try {
  CHECK_H(h);
  if (!body || !group || !sy) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(network_ready(h, "lbmdem_network_device"));
  *body = h->net.body;
  *group = h->net.group;
  *sy = h->L.sy;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_network_bodies(lbmdem_handle* h, lbmdem_net_body* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(network_ready(h, "lbmdem_download_network_bodies"));
  return stage_table(h, "lbmdem_download_network_bodies", "bodies", h->net.bodies, sizeof *out, h->net.nbodies, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_network_groups(lbmdem_handle* h, lbmdem_net_group* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(network_ready(h, "lbmdem_download_network_groups"));
  return stage_table(h, "lbmdem_download_network_groups", "groups", h->net.groups, sizeof *out, h->net.ngroups, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_network_links(lbmdem_handle* h, int level, lbmdem_net_link* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  if (level != 0 && level != 1)
    return fail(LBMDEM_EINVAL, "lbmdem_download_network_links: level must be 0 (between bodies) or 1 (between groups) (%d)", level);
  RC_TRY(network_ready(h, "lbmdem_download_network_links"));
  return stage_table(h, "lbmdem_download_network_links", "links", h->net.links[level], sizeof *out, h->net.nlinks[level], out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_network(lbmdem_handle* h, const char* dir, int nfile, int merge, int plane) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_network"));
  const LatticeView& L = h->L;
  long counts[LBMDEM_NETWORK_COUNTS], nb = 0, ng = 0, nl = 0;
  RC_TRY(lbmdem_network_compute(h, nullptr, merge, 0, counts));
  RC_TRY(lbmdem_download_network_bodies(h, nullptr, 0, &nb));
  RC_TRY(lbmdem_download_network_groups(h, nullptr, 0, &ng));
  RC_TRY(lbmdem_download_network_links(h, 1, nullptr, 0, &nl));
  std::vector<lbmdem_net_body> bodies((size_t)nb);
  std::vector<lbmdem_net_group> groups((size_t)ng);
  std::vector<lbmdem_net_link> links((size_t)nl);
  if (nb > 0) RC_TRY(lbmdem_download_network_bodies(h, bodies.data(), nb, &nb));
  if (ng > 0) RC_TRY(lbmdem_download_network_groups(h, groups.data(), ng, &ng));
  if (nl > 0) RC_TRY(lbmdem_download_network_links(h, 1, links.data(), nl, &nl));
  std::vector<int> planes;
  const size_t cnt = (size_t)L.lx * L.ly;
  if (plane) {
    planes.resize(2 * cnt);
    RC_TRY(lbmdem_download_network(h, planes.data(), planes.data() + cnt));
  }
  return lbmdem_write_network_files(dir, nfile, L.lx, L.ly, h->n, merge, plane, plane ? planes.data() : nullptr,
                                    plane ? planes.data() + cnt : nullptr, nb > 0 ? bodies.data() : nullptr, nb,
                                    ng > 0 ? groups.data() : nullptr, ng, nl > 0 ? links.data() : nullptr, nl, counts,
                                    h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_network_output(lbmdem_handle* h, int on, int merge, int plane) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_network_output"));
    if (merge < -1) return fail(LBMDEM_EINVAL, "lbmdem_set_network_output: merge must be -1 (no merging) or a difference of radii >= 0 (%d)", merge);
    h->network_merge = merge;
    h->network_plane = plane != 0;
  }
  h->network_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
