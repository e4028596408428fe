// lbm_clearance.hip -- how wide is the pore space: the exact squared Euclidean distance from every fluid node of the obstacle map
// to the nearest position that is not fluid, that position's owner, the pore-size histogram, per owner the fluid nodes it has, and
// the throats -- per pair of owners whose regions meet, the length of the ridge between them and its narrowest place
// (lbmdem_clearance_compute, lbmdem_download_clearance, lbmdem_clearance_device, lbmdem_download_clearance_hist,
// lbmdem_download_clearance_owners, lbmdem_clearance_owners_device, lbmdem_download_throats, lbmdem_write_clearance,
// lbmdem_set_clearance_output, lbmdem_write_clearance_files; include/lbmdem_hip.h, "Pore clearance", has the contract in full).
// Every result is an integer and every tie has a rule, so nothing depends on the order anything happens in. Nothing here is on the
// step path: the kernels only read the map and write to the handle's ClearanceStage, and nothing is allocated or launched before
// the first compute.
//
// One packed 64-bit key per node, distance squared << 32 | owner: the smaller key is the nearer position and, among equals, the
// smaller owner (a grain before the wall, n). In the device layout (node = x*sy + y), on the handle's stream:
//   k_ce_init     the histogram, the owners' table and the census words;
//   k_ce_row      one wavefront per row x, lanes along y in chunks of 64: a running maximum of (position, owner) upward and a
//                 running minimum downward by wave shifts give the nearest non-fluid position of the row on either side -- the
//                 positions -1 and ly outside the lattice seed them with the owner n -- and the key g^2 << 32 | owner of the nearer;
//   k_ce_col      lanes along y, 32 rows per workgroup: a node walks x' = x -+ 1, x -+ 2, .. and keeps the minimum of
//                 (dx^2 << 32) + key(x', y); rows outside the lattice give dx^2 << 32 | n. The walk ends at the first dx whose
//                 square exceeds the best distance (a square EQUAL to it may still bring a smaller owner), and that is exact: the
//                 nearest non-fluid position within row x' is that row's nearest along y. It writes d2 and owner, counts the
//                 histogram (the lanes of a wavefront that share a bin first, LDS bins per workgroup, then 64-bit atomics) and
//                 the owners' table (the lanes that share an owner first, an LDS slot per owner modulo 64, then atomics), and the
//                 sums of the census;
//   k_ce_count, a scan, k_ce_emit   the ridge: per pair of 4-adjacent fluid nodes with different owners one record
//                 (pair key, clearance << pbits | node), in node order;
//   two stable hipcub::DeviceRadixSort passes, by value and then by pair, a run-length encode and a scan of the run lengths;
//   k_ce_throats  one record per run: its pair, its length, and from its first record the smallest clearance and that one's
//                 smallest node;
//   k_ce_census   the counts over the throats and the owners.
// Single launches, no host-driven rounds, no workgroup waits for another, integer atomics only, no floating point anywhere. Every
// loop has the bound its comment states.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both. Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h), MemPool (lbm_mem.h) for the
// scratch kept on the handle, OutFile (lbm_outfile.h) for the files; what the pore stages share, lbm_stage.h.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_stage.h"

#include <limits.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

constexpr int CE_SIDE_MAX = 32768;   // d2 <= ((min(lx, ly) + 1) / 2)^2 < 2^31, a node's index < 2^30

#ifndef LBMDEM_SINGLE_PRECISION
typedef unsigned long long ce_u64;
constexpr int CE_THREADS = 256;
constexpr int CE_ROWS = 32;        // rows of a workgroup of the column pass
constexpr int CE_LDS_BINS = 2048;  // histogram bins a workgroup keeps in LDS; the bins beyond go to global memory at once
constexpr int CE_SLOTS = 64;       // LDS slots of the owners' table, by owner modulo CE_SLOTS
// ClearanceStage::words
enum : int { CE_W_FLUID = 0, CE_W_SUM, CE_W_BEST, CE_W_GRAIN_THROATS, CE_W_NARROWEST, CE_W_OWNERLESS, CE_WORDS };

struct CeJob {
  const int* M;      // the map, device layout
  int lx, ly, sy, n;
  long N;            // lx * sy
  ce_u64* key;       // [lx][sy] the row pass' result
  int* d2;           // [lx][sy]
  int* owner;        // [lx][sy]
  ce_u64* hist;      // [hbins]
  int hbins;
  ce_u64* owned;     // [n + 1]
  int* d2max;        // [n + 1]
  ce_u64* words;
  ce_u64* cnt;       // [nblocks + 1] ridge edges per block of CE_THREADS nodes
  ce_u64* off;       // [nblocks + 1] their scan
  long nblocks;
  ce_u64* rk;        // [nedges] pair keys, lo * (n + 1) + hi
  ce_u64* rv;        // [nedges] c << pbits | p
  long nedges;
  int pbits;         // bits of a host index
  const ce_u64* uniq;   // [nthroats] the pair keys, ascending
  const int* runs;      // [nthroats] their run lengths
  const int* offs;      // [nthroats] the runs' first records
  lbmdem_throat* table;
  long nthroats;
};

__global__ __launch_bounds__(CE_THREADS) void k_ce_init(const CeJob J) {
  const int i = blockIdx.x * CE_THREADS + threadIdx.x;
  if (i < J.hbins) J.hist[i] = 0;
  if (i <= J.n) { J.owned[i] = 0; J.d2max[i] = -1; }
  if (i < CE_WORDS) J.words[i] = i == CE_W_NARROWEST ? ~0ull : 0ull;
}

// One wavefront per row. (position + 1) << 32 | owner, so that the seed below the lattice, position -1, is the word n itself and a
// fluid node's 0 is below every candidate.
__global__ __launch_bounds__(CE_THREADS) void k_ce_row(const CeJob J) {
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * (CE_THREADS / 64) + (threadIdx.x >> 6);
  if (x >= J.lx) return;   // (the whole wavefront)
  const int ly = J.ly;
  const int* const Mrow = J.M + (long)x * J.sy;
  ce_u64* const K = J.key + (long)x * J.sy;
  const int chunks = (ly + 63) / 64;
  ce_u64 carry = (ce_u64)(unsigned)J.n;
  for (int c = 0; c < chunks; ++c) {   // upward: the nearest non-fluid position at or below y
    const int y = c * 64 + lane;
    const int m = y < ly ? Mrow[y] : -1;   // (the pad columns are never read)
    ce_u64 v = m >= 0 ? ((ce_u64)(unsigned)(y + 1) << 32 | (unsigned)m) : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const ce_u64 o = __shfl_up(v, d);
      if (lane >= d && o > v) v = o;
    }
    if (carry > v) v = carry;
    if (y < ly) K[y] = v;
    carry = __shfl(v, 63);
  }
  carry = (ce_u64)(unsigned)(ly + 1) << 32 | (unsigned)J.n;
  for (int c = chunks - 1; c >= 0; --c) {   // downward: the nearest at or above y, and the key of the nearer of the two
    const int y = c * 64 + lane;
    const int m = y < ly ? Mrow[y] : -1;
    ce_u64 v = m >= 0 ? ((ce_u64)(unsigned)(y + 1) << 32 | (unsigned)m) : ~0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const ce_u64 o = __shfl_down(v, d);
      if (lane + d < 64 && o < v) v = o;
    }
    if (carry < v) v = carry;
    carry = __shfl(v, 0);
    if (y < ly) {
      const ce_u64 dn = K[y];   // (this lane's own store of the first loop)
      const unsigned gd = (unsigned)(y + 1) - (unsigned)(dn >> 32), gu = (unsigned)(v >> 32) - (unsigned)(y + 1);
      const unsigned od = (unsigned)dn, ou = (unsigned)v;
      const unsigned g = gd < gu ? gd : gu;
      const unsigned o = gd < gu ? od : gu < gd ? ou : (od < ou ? od : ou);
      K[y] = (ce_u64)(g * g) << 32 | o;   // g <= 32768
    }
  }
}

// floor(sqrt(v)) in integers, 16 rounds
__device__ __forceinline__ int ce_isqrt(unsigned v) {
  unsigned r = 0;
#pragma unroll
  for (unsigned b = 1u << 15; b; b >>= 1) {
    const unsigned t = r | b;
    if (t * t <= v) r = t;
  }
  return (int)r;
}

__device__ __forceinline__ ce_u64 ce_wave_sum(ce_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}
__device__ __forceinline__ ce_u64 ce_wave_max(ce_u64 v) {
  for (int m = 32; m >= 1; m >>= 1) { const ce_u64 o = __shfl_xor(v, m); v = o > v ? o : v; }
  return v;
}

__global__ __launch_bounds__(CE_THREADS) void k_ce_col(const CeJob J) {
  __shared__ unsigned s_hist[CE_LDS_BINS];
  __shared__ int s_own[CE_SLOTS], s_max[CE_SLOTS];
  __shared__ ce_u64 s_cnt[CE_SLOTS];
  __shared__ ce_u64 s_fluid, s_sum, s_best;
  for (int i = threadIdx.x; i < CE_LDS_BINS; i += CE_THREADS) s_hist[i] = 0;
  if (threadIdx.x < CE_SLOTS) { s_own[threadIdx.x] = -1; s_max[threadIdx.x] = -1; s_cnt[threadIdx.x] = 0; }
  if (threadIdx.x == 0) { s_fluid = 0; s_sum = 0; s_best = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * CE_THREADS + threadIdx.x;
  const int lx = J.lx, ly = J.ly, sy = J.sy;
  const ce_u64 wall = (ce_u64)(unsigned)J.n;
  const bool inside = y < ly;
  ce_u64 nfluid = 0, sum = 0, top = 0;   // this lane's, over its rows
  for (int r = 0; r < CE_ROWS; ++r) {
    const int x = blockIdx.y * CE_ROWS + r;
    if (x >= lx) break;   // (the whole workgroup)
    const long node = (long)x * sy + y;
    int d2 = 0, own = -1;
    if (inside) {
      ce_u64 best = J.key[node];
      // Ends within max(x + 1, lx - x) + 1 steps: at dx = max(x + 1, lx - x) both rows lie outside the lattice and are not fluid,
      // so the best distance is at most dx^2 and the next square exceeds it.
      for (int dx = 1; dx <= lx + 1; ++dx) {
        const ce_u64 dd = (ce_u64)dx * (ce_u64)dx;
        if (dd > (best >> 32)) break;
        const ce_u64 a = x - dx >= 0 ? (dd << 32) + J.key[node - (long)dx * sy] : (dd << 32 | wall);
        const ce_u64 b = x + dx < lx ? (dd << 32) + J.key[node + (long)dx * sy] : (dd << 32 | wall);
        const ce_u64 ab = a < b ? a : b;
        best = ab < best ? ab : best;
      }
      d2 = (int)(best >> 32);
      own = (int)(unsigned)best;
    }
    if (y < sy) { J.d2[node] = d2; J.owner[node] = own; }   // (the pad columns: 0 and -1)
    const bool fluid = d2 > 0;
    const int k = ce_isqrt((unsigned)d2);
    if (inside) {
      const ce_u64 mine = (ce_u64)(unsigned)d2 << 32 | (ce_u64)(0xFFFFFFFFu - (unsigned)((long)x * ly + y));   // the smaller index wins
      top = mine > top ? mine : top;
    }
    nfluid += fluid;
    sum += (ce_u64)(unsigned)d2;
    // the lanes that share a bin, then those that share an owner: every round retires its leader's lanes, 64 rounds at most
    ce_u64 todo = __ballot(fluid);
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int kk = __shfl(k, lead);
      const ce_u64 same = __ballot(fluid && k == kk);
      if (lane == lead) {
        if (kk < CE_LDS_BINS) atomicAdd(&s_hist[kk], (unsigned)__popcll(same));
        else if (kk < J.hbins) atomicAdd(&J.hist[kk], (ce_u64)__popcll(same));
      }
      todo &= ~same;
    }
    todo = __ballot(fluid);
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int oo = __shfl(own, lead);
      const bool with = fluid && own == oo;
      const ce_u64 same = __ballot(with);
      const int dmax = (int)ce_wave_max(with ? (ce_u64)(unsigned)d2 : 0ull);
      if (lane == lead && oo >= 0 && oo <= J.n) {
        const int slot = oo & (CE_SLOTS - 1);
        const int held = atomicCAS(&s_own[slot], -1, oo);
        if (held == -1 || held == oo) {
          atomicAdd(&s_cnt[slot], (ce_u64)__popcll(same));
          atomicMax(&s_max[slot], dmax);
        } else {
          atomicAdd(&J.owned[oo], (ce_u64)__popcll(same));
          atomicMax(&J.d2max[oo], dmax);
        }
      }
      todo &= ~same;
    }
  }
  nfluid = ce_wave_sum(nfluid);
  sum = ce_wave_sum(sum);
  top = ce_wave_max(top);
  if (lane == 0) {
    if (nfluid) atomicAdd(&s_fluid, nfluid);
    if (sum) atomicAdd(&s_sum, sum);
    atomicMax(&s_best, top);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CE_LDS_BINS && i < J.hbins; i += CE_THREADS)
    if (s_hist[i]) atomicAdd(&J.hist[i], (ce_u64)s_hist[i]);
  if (threadIdx.x < CE_SLOTS && s_own[threadIdx.x] >= 0) {
    atomicAdd(&J.owned[s_own[threadIdx.x]], s_cnt[threadIdx.x]);
    atomicMax(&J.d2max[s_own[threadIdx.x]], s_max[threadIdx.x]);
  }
  if (threadIdx.x == 0) {
    if (s_fluid) atomicAdd(&J.words[CE_W_FLUID], s_fluid);
    if (s_sum) atomicAdd(&J.words[CE_W_SUM], s_sum);
    atomicMax(&J.words[CE_W_BEST], s_best);
  }
}

// The ridge edges that start at a device node: towards (x, y + 1) and towards (x + 1, y), in that order (ascending q). A node is
// fluid exactly where d2 > 0; the pad columns hold 0.
__device__ __forceinline__ int ce_edges_of(const CeJob& J, long node, ce_u64* rk, ce_u64* rv) {
  const int x = (int)(node / J.sy), y = (int)(node % J.sy);
  if (node >= J.N || y >= J.ly) return 0;
  const int d = J.d2[node];
  if (d <= 0) return 0;
  const int o = J.owner[node];
  const ce_u64 p = (ce_u64)((long)x * J.ly + y);
  int cnt = 0;
  if (y + 1 < J.ly) {
    const int d1 = J.d2[node + 1], o1 = J.owner[node + 1];
    if (d1 > 0 && o1 != o) {
      const int lo = o < o1 ? o : o1, hi = o < o1 ? o1 : o;
      rk[cnt] = (ce_u64)lo * (ce_u64)(J.n + 1) + (ce_u64)hi;
      rv[cnt] = (ce_u64)(unsigned)(d > d1 ? d : d1) << J.pbits | p;
      ++cnt;
    }
  }
  if (x + 1 < J.lx) {
    const int d1 = J.d2[node + J.sy], o1 = J.owner[node + J.sy];
    if (d1 > 0 && o1 != o) {
      const int lo = o < o1 ? o : o1, hi = o < o1 ? o1 : o;
      rk[cnt] = (ce_u64)lo * (ce_u64)(J.n + 1) + (ce_u64)hi;
      rv[cnt] = (ce_u64)(unsigned)(d > d1 ? d : d1) << J.pbits | p;
      ++cnt;
    }
  }
  return cnt;
}

__global__ __launch_bounds__(CE_THREADS) void k_ce_count(const CeJob J) {
  __shared__ ce_u64 part[CE_THREADS / 64];
  const long node = (long)blockIdx.x * CE_THREADS + threadIdx.x;
  ce_u64 rk[2], rv[2];
  const ce_u64 mine = ce_wave_sum((ce_u64)ce_edges_of(J, node, rk, rv));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    ce_u64 s = 0;
    for (int w = 0; w < CE_THREADS / 64; ++w) s += part[w];
    J.cnt[blockIdx.x] = s;
    if (blockIdx.x == 0) J.cnt[J.nblocks] = 0;   // the scan's last item
  }
}

__global__ __launch_bounds__(CE_THREADS) void k_ce_emit(const CeJob J) {
  typedef hipcub::BlockScan<int, CE_THREADS> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const long node = (long)blockIdx.x * CE_THREADS + threadIdx.x;
  ce_u64 rk[2], rv[2];
  const int mine = ce_edges_of(J, node, rk, rv);
  int before = 0;
  Scan(tmp).ExclusiveSum(mine, before);
  const long at = (long)J.off[blockIdx.x] + before;
  for (int k = 0; k < mine; ++k)
    if (at + k < J.nedges) {   // (always: nedges is the scan's total)
      J.rk[at + k] = rk[k];
      J.rv[at + k] = rv[k];
    }
}

// One throat per run of equal pairs; the records of a run ascend by (clearance, node).
__global__ __launch_bounds__(CE_THREADS) void k_ce_throats(const CeJob J) {
  const long t = (long)blockIdx.x * CE_THREADS + threadIdx.x;
  if (t >= J.nthroats) return;
  const ce_u64 key = J.uniq[t];
  const long first = J.offs[t];
  const ce_u64 v = first >= 0 && first < J.nedges ? J.rv[first] : 0ull;   // (always inside)
  lbmdem_throat e;
  e.lo = (int)(key / (ce_u64)(J.n + 1));
  e.hi = (int)(key % (ce_u64)(J.n + 1));
  e.edges = J.runs[t];
  e.c_min = (int)(v >> J.pbits);
  e.node = (int)(v & ((1ull << J.pbits) - 1ull));
  J.table[t] = e;
}

__global__ __launch_bounds__(CE_THREADS) void k_ce_census(const CeJob J) {
  const long i = (long)blockIdx.x * CE_THREADS + threadIdx.x;
  bool gg = false, none = false;
  ce_u64 c = ~0ull;
  if (i < J.nthroats) {
    const lbmdem_throat e = J.table[i];
    gg = e.hi < J.n;
    if (gg) c = (ce_u64)(unsigned)e.c_min;
  }
  if (i < J.n) none = J.owned[i] == 0;
  for (int m = 32; m >= 1; m >>= 1) { const ce_u64 o = __shfl_xor(c, m); c = o < c ? o : c; }
  const ce_u64 ngg = __popcll(__ballot(gg)), nnone = __popcll(__ballot(none));
  if ((threadIdx.x & 63) == 0) {
    if (ngg) { atomicAdd(&J.words[CE_W_GRAIN_THROATS], ngg); atomicMin(&J.words[CE_W_NARROWEST], c); }
    if (nnone) atomicAdd(&J.words[CE_W_OWNERLESS], nnone);
  }
}

long ce_isqrt_host(long v) { long r = 0; for (long b = 1L << 15; b; b >>= 1) if ((r | b) * (r | b) <= v) r |= b; return r; }

// what depends on the lattice and on n, once
int clearance_stage(lbmdem_handle* h) {
  auto& V = h->clr;
  if (V.words) return LBMDEM_OK;
  const size_t N = (size_t)h->L.lx * h->L.sy;
  const long nb = stage_blocks((long)N, CE_THREADS);
  const int side = h->L.lx < h->L.ly ? h->L.lx : h->L.ly;
  V.hbins = (side + 1) / 2 + 2;   // isqrt(d2) <= (min(lx, ly) + 1) / 2
  HIP_TRY(h->mem.dev(&V.key, N));
  HIP_TRY(h->mem.dev(&V.d2, N));
  HIP_TRY(h->mem.dev(&V.owner, N));
  HIP_TRY(h->mem.dev(&V.hist, (size_t)V.hbins));
  HIP_TRY(h->mem.dev(&V.owned, (size_t)h->n + 1));
  HIP_TRY(h->mem.dev(&V.d2max, (size_t)h->n + 1));
  HIP_TRY(h->mem.dev(&V.cnt, 2 * ((size_t)nb + 1)));
  HIP_TRY(h->mem.dev(&V.nruns, (size_t)1));
  HIP_TRY(h->mem.dev(&V.words, (size_t)CE_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

int clearance_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  if (!h->clr.at.current(h))
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_clearance_compute has been made for the map as it is now", who);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_clearance_files(const char* dir, int nfile, int lx, int ly, int plane, const int* d2, const int* owner,
                                 const lbmdem_throat* table, long ntable, const long* hist, long nhist, int n, const long* owned,
                                 const int* d2max, const long* counts10, double t) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (n < 1 || ntable < 0 || (ntable > 0 && !table) || nhist < 1 || !hist || !owned || !d2max || !counts10 || (plane && (!d2 || !owner)))
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_clearance_files arguments");
  if (lx < 2 || ly < 2 || lx > CE_SIDE_MAX || ly > CE_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_write_clearance_files: the lattice is %d x %d", lx, ly);
  const long cnt = (long)lx * ly;
  if (plane)
    for (long k = 0; k < cnt; ++k) {
      if (d2[k] < 0) return fail(LBMDEM_EINVAL, "lbmdem_write_clearance_files: d2[%ld][%ld] = %d is negative", k / ly, k % ly, d2[k]);
      if (owner[k] < 0 || owner[k] > n)
        return fail(LBMDEM_EINVAL, "lbmdem_write_clearance_files: owner[%ld][%ld] = %d is outside [0, %d]", k / ly, k % ly, owner[k], n);
    }
  for (long k = 0; k < ntable; ++k) {
    const lbmdem_throat& e = table[k];
    const bool ascends = k == 0 || e.lo > table[k - 1].lo || (e.lo == table[k - 1].lo && e.hi > table[k - 1].hi);
    if (e.lo < 0 || e.lo >= e.hi || e.hi > n || !ascends)
      return fail(LBMDEM_EINVAL, "lbmdem_write_clearance_files: entry %ld of the table has the pair (%d, %d): the pairs ascend, "
                                 "0 <= lo < hi <= %d", k, e.lo, e.hi, n);
  }
  OutFile F;
  RC_TRY(F.open("w", dir, "throats%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# lx %d ly %d n %d\n", lx, ly, n);
  fprintf(fp, "# lo hi edges c_min node\n");
  for (long k = 0; k < ntable; ++k) {
    const lbmdem_throat& e = table[k];
    fprintf(fp, "%d %d %d %d %d\n", e.lo, e.hi, e.edges, e.c_min, e.node);
  }
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "clearance_hist%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# k nodes\n");
  for (long k = 0; k < nhist; ++k) fprintf(fp, "%ld %ld\n", k, hist[k]);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "clearance_owners%.6i.dat", nfile));
  fp = F.fp;
  fprintf(fp, "# owner owned d2max\n");
  for (int i = 0; i <= n; ++i) fprintf(fp, "%d %ld %d\n", i, owned[i], d2max[i]);
  RC_TRY(F.close());
  if (plane) {
    const int* const planes[2] = {d2, owner};
    const char* const names[2] = {"d2", "owner"};
    RC_TRY(stage_write_int_planes(F, dir, nfile, "clearance%.6i.vtk", "lbmdem pore clearance", lx, ly, names, planes, 2));
  }
  return stage_append_row(F, dir, "clearance.data",
                          "# t fluid_nodes d2_max d2_max_node sum_d2 ridge_edges throats grain_throats narrowest_c ownerless_grains kmax",
                          t, counts10, LBMDEM_CLEARANCE_COUNTS);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_clearance_compute(lbmdem_handle* h, const int*, long, long*) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_download_clearance(lbmdem_handle* h, int*, int*) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_clearance_device(lbmdem_handle* h, const int**, const int**, int*) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_download_clearance_hist(lbmdem_handle* h, long*, long, long*) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_download_clearance_owners(lbmdem_handle* h, long*, int*) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_clearance_owners_device(lbmdem_handle* h, const long**, const int**) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_download_throats(lbmdem_handle* h, lbmdem_throat*, long, long*) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_write_clearance(lbmdem_handle* h, const char*, int, int) { SP_REFUSE(h, "the pore clearance analysis"); }
int lbmdem_set_clearance_output(lbmdem_handle* h, int, int) { SP_REFUSE(h, "the pore clearance analysis"); }
#else

int lbmdem_clearance_compute(lbmdem_handle* h, const int* map, long max_edges, long* counts10) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts10) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_clearance_compute"));
  const LatticeView& L = h->L;
  const int lx = L.lx, ly = L.ly, sy = L.sy, n = h->n;
  if (lx > CE_SIDE_MAX || ly > CE_SIDE_MAX)
    return fail(LBMDEM_EINVAL, "lbmdem_clearance_compute: a lattice of %d x %d nodes has a side above %d: the squared distances are "
                               "32-bit integers", lx, ly, CE_SIDE_MAX);
  RC_TRY(stage_check_max_edges("lbmdem_clearance_compute", max_edges));
  auto& V = h->clr;
  V.at.valid = false;
  RC_TRY(stage_check_map("lbmdem_clearance_compute", map, lx, ly, n));
  RC_TRY(clearance_stage(h));
  const hipStream_t st = h->stream;
  const long N = (long)lx * sy;
  CeJob J{};
  J.M = reader_obst(h);
  if (map) {
    RC_TRY(stage_upload_map(h, &V.map, map));
    J.M = V.map;
  }
  J.lx = lx; J.ly = ly; J.sy = sy; J.n = n;
  J.N = N;
  J.key = V.key; J.d2 = V.d2; J.owner = V.owner;
  J.hist = V.hist; J.hbins = V.hbins;
  J.owned = V.owned; J.d2max = V.d2max;
  J.words = V.words;
  J.nblocks = stage_blocks(N, CE_THREADS);
  J.cnt = V.cnt; J.off = V.cnt + J.nblocks + 1;
  J.pbits = stage_bits((unsigned long long)((long)lx * ly - 1));
  const int need = V.hbins > n + 1 ? V.hbins : n + 1;
  hipLaunchKernelGGL(k_ce_init, dim3((unsigned)stage_blocks(need > CE_WORDS ? need : CE_WORDS, CE_THREADS)), dim3(CE_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_ce_row, dim3((unsigned)stage_blocks(lx, CE_THREADS / 64)), dim3(CE_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_ce_col, dim3((unsigned)stage_blocks(sy, CE_THREADS), (unsigned)stage_blocks(lx, CE_ROWS)), dim3(CE_THREADS), 0, st, J);
  hipLaunchKernelGGL(k_ce_count, dim3((unsigned)J.nblocks), dim3(CE_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  size_t b = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, J.cnt, J.off, (int)(J.nblocks + 1), st));
  HIP_TRY(h->mem.grow(&V.tmp, &V.tmp_bytes, (long)b));
  b = (size_t)V.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(V.tmp, b, J.cnt, J.off, (int)(J.nblocks + 1), st));
  unsigned long long nedges = 0;
  HIP_TRY(hipMemcpyAsync(&nedges, J.off + J.nblocks, sizeof nedges, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // (the caller's map has been read too)
  if (nedges > (unsigned long long)(max_edges > 0 ? max_edges : (long)INT_MAX))
    return fail(LBMDEM_EINVAL, "lbmdem_clearance_compute: the ridge has %llu edges, max_edges is %ld", nedges,
                max_edges > 0 ? max_edges : (long)INT_MAX);
  const int E = (int)nedges;
  int T = 0;
  if (E > 0) {
    if (V.rec_cap < E) {   // the records' blocks go and come together; rec_cap says so only once all three are there
      const long want = (long)E + E / 4 + 64;
      V.rec_cap = 0;
      h->mem.release(V.rec); V.rec = nullptr;
      h->mem.release(V.uniq); V.uniq = nullptr;
      h->mem.release(V.runs); V.runs = nullptr;
      HIP_TRY(h->mem.dev(&V.rec, 4 * (size_t)want));
      HIP_TRY(h->mem.dev(&V.uniq, (size_t)want));
      HIP_TRY(h->mem.dev(&V.runs, 2 * (size_t)want));
      V.rec_cap = want;
    }
    const long cap = V.rec_cap;
    ce_u64 *const rk0 = V.rec, *const rk1 = V.rec + cap, *const rv0 = V.rec + 2 * cap, *const rv1 = V.rec + 3 * cap;
    int *const runs = V.runs, *const offs = V.runs + cap;
    J.rk = rk0; J.rv = rv0; J.nedges = E;
    hipLaunchKernelGGL(k_ce_emit, dim3((unsigned)J.nblocks), dim3(CE_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    const int side = lx < ly ? lx : ly;
    const long dtop = (long)((side + 1) / 2 + 1) * ((side + 1) / 2 + 1);
    const int vbits = J.pbits + stage_bits((unsigned long long)dtop);
    const int kbits = stage_bits((unsigned long long)(n + 1) * (unsigned long long)(n + 1));
    size_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, rv0, rv1, rk0, rk1, E, 0, vbits, st));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b2, rk1, rk0, rv1, rv0, E, 0, kbits, st));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, b3, rk0, V.uniq, runs, V.nruns, E, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b4, runs, offs, E, st));
    b = b1 > b2 ? b1 : b2; b = b > b3 ? b : b3; b = b > b4 ? b : b4;
    HIP_TRY(h->mem.grow(&V.tmp, &V.tmp_bytes, (long)b));
    b = (size_t)V.tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(V.tmp, b, rv0, rv1, rk0, rk1, E, 0, vbits, st));   // by (clearance, node)
    b = (size_t)V.tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(V.tmp, b, rk1, rk0, rv1, rv0, E, 0, kbits, st));   // stable: then by pair
    b = (size_t)V.tmp_bytes;
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(V.tmp, b, rk0, V.uniq, runs, V.nruns, E, st));
    HIP_TRY(hipMemcpyAsync(&T, V.nruns, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    b = (size_t)V.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(V.tmp, b, runs, offs, T, st));
    HIP_TRY(h->mem.grow(&V.table, &V.table_cap, (long)T + T / 4 + 64));
    J.uniq = V.uniq; J.runs = runs; J.offs = offs;
    J.table = V.table; J.nthroats = T;
    hipLaunchKernelGGL(k_ce_throats, dim3((unsigned)stage_blocks(T, CE_THREADS)), dim3(CE_THREADS), 0, st, J);
  }
  J.table = V.table; J.nthroats = T;
  hipLaunchKernelGGL(k_ce_census, dim3((unsigned)stage_blocks(T > n ? T : n, CE_THREADS)), dim3(CE_THREADS), 0, st, J);
  HIP_TRY(hipGetLastError());
  unsigned long long w[CE_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const long d2_max = (long)(w[CE_W_BEST] >> 32);
  counts10[0] = (long)w[CE_W_FLUID];
  counts10[1] = d2_max;
  counts10[2] = (long)(0xFFFFFFFFull - (w[CE_W_BEST] & 0xFFFFFFFFull));
  counts10[3] = (long)w[CE_W_SUM];
  counts10[4] = E;
  counts10[5] = T;
  counts10[6] = (long)w[CE_W_GRAIN_THROATS];
  counts10[7] = w[CE_W_GRAIN_THROATS] ? (long)w[CE_W_NARROWEST] : -1;
  counts10[8] = (long)w[CE_W_OWNERLESS];
  counts10[9] = ce_isqrt_host(d2_max);
  V.nedges = E; V.nthroats = T; V.kmax = (int)counts10[9];
  V.own = map == nullptr;
  V.gen += 1;
  V.at.set(h);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_clearance(lbmdem_handle* h, int* d2, int* owner) try {
  CHECK_H(h);
  if (!d2 && !owner) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(clearance_ready(h, "lbmdem_download_clearance"));
  if (d2) RC_TRY(stage_download_plane(h, d2, h->clr.d2));
  if (owner) RC_TRY(stage_download_plane(h, owner, h->clr.owner));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_clearance_device(lbmdem_handle* h, const int** d2, const int** owner, int* sy) try {
  CHECK_H(h);
  if (!d2 || !owner || !sy) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(clearance_ready(h, "lbmdem_clearance_device"));
  *d2 = h->clr.d2;
  *owner = h->clr.owner;
  *sy = h->L.sy;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_clearance_hist(lbmdem_handle* h, long* hist, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !hist)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(clearance_ready(h, "lbmdem_download_clearance_hist"));
  return stage_table(h, "lbmdem_download_clearance_hist", "bins", h->clr.hist, sizeof *hist, (long)h->clr.kmax + 1, hist, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_clearance_owners(lbmdem_handle* h, long* owned, int* d2max) try {
  CHECK_H(h);
  RC_TRY(clearance_ready(h, "lbmdem_download_clearance_owners"));
  const size_t m = (size_t)h->n + 1;   // (a fixed length and no cap: not a stage_table)
  if (owned) HIP_TRY(hipMemcpyAsync(owned, h->clr.owned, sizeof(long) * m, hipMemcpyDeviceToHost, h->stream));
  if (d2max) HIP_TRY(hipMemcpyAsync(d2max, h->clr.d2max, sizeof(int) * m, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_clearance_owners_device(lbmdem_handle* h, const long** owned, const int** d2max) try {
  CHECK_H(h);
  RC_TRY(clearance_ready(h, "lbmdem_clearance_owners_device"));
  if (owned) *owned = reinterpret_cast<const long*>(h->clr.owned);
  if (d2max) *d2max = h->clr.d2max;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_throats(lbmdem_handle* h, lbmdem_throat* out, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0 || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(clearance_ready(h, "lbmdem_download_throats"));
  return stage_table(h, "lbmdem_download_throats", "throats", h->clr.table, sizeof *out, h->clr.nthroats, out, cap, count);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_clearance(lbmdem_handle* h, const char* dir, int nfile, int plane) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  RC_TRY(whole_handle(h, "lbmdem_write_clearance"));
  const LatticeView& L = h->L;
  const size_t m = (size_t)h->n + 1;
  long counts[LBMDEM_CLEARANCE_COUNTS], ntable = 0, nhist = 0;
  RC_TRY(lbmdem_clearance_compute(h, nullptr, 0, counts));
  RC_TRY(lbmdem_download_throats(h, nullptr, 0, &ntable));
  std::vector<lbmdem_throat> table((size_t)ntable);
  if (ntable > 0) RC_TRY(lbmdem_download_throats(h, table.data(), ntable, &ntable));
  RC_TRY(lbmdem_download_clearance_hist(h, nullptr, 0, &nhist));
  std::vector<long> hist((size_t)nhist), owned(m);
  RC_TRY(lbmdem_download_clearance_hist(h, hist.data(), nhist, &nhist));
  std::vector<int> d2max(m), planes;
  RC_TRY(lbmdem_download_clearance_owners(h, owned.data(), d2max.data()));
  const size_t cnt = (size_t)L.lx * L.ly;
  if (plane) {
    planes.resize(2 * cnt);
    RC_TRY(lbmdem_download_clearance(h, planes.data(), planes.data() + cnt));
  }
  return lbmdem_write_clearance_files(dir, nfile, L.lx, L.ly, plane, plane ? planes.data() : nullptr, plane ? planes.data() + cnt : nullptr,
                                      ntable > 0 ? table.data() : nullptr, ntable, hist.data(), nhist, h->n, owned.data(),
                                      d2max.data(), counts, h->nbsteps * h->cfg.dt);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_clearance_output(lbmdem_handle* h, int on, int plane) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_clearance_output"));
    h->clearance_plane = plane != 0;
  }
  h->clearance_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
