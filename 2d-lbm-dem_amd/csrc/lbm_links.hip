// lbm_links.hip -- the boundary-link export (lbmdem_geometry_stats, lbmdem_download_act, lbmdem_download_links,
// lbmdem_download_geometry_obst, lbmdem_write_obst, lbmdem_write_obst_files; include/lbmdem_hip.h): the two arrays of
// obst_construction (main.c:991-1065) that the library never stores -- act[x][y] and delta[x][y][q] -- derived once more from the
// obstacle map and the centres of the most recent rasterisation, in the order obst_writing (main.c:1601-1641) prints them:
// y outer, x inner, q = 1..8. Nothing here is on the step path: the kernels only read the handle's state.
//
// An EFFECTIVE LINK is a (node P, direction q) that the reference's bounce-back loop (main.c:1154-1222) takes into its
// interpolation branch: P an interior node of a grain, act[P] == 1, obst[P + e_q] == -1. Its delta is link_delta<q> of P against
// the owner's reduced disc -- bit for bit the reference's delta[P][q], the owner being the last grain to paint P. The reference's
// delta array can hold further non-zero entries that its loop never reads (left by a lower-index disc at a node, or towards a
// neighbour, that a higher-index disc painted afterwards): those are no links and are not exported.
//
// Three steps on the handle's stream, the order fixed without atomics:
//   k_links_count  act of every node (bytes, [x][y]), the number of effective links per cell -- one y, 64 consecutive x --, the
//                  six counters of lbmdem_geometry_stats;
//   an exclusive scan of the cells in file order (hipcub::DeviceScan);
//   k_links_emit   the links of every cell once more, stored at the scanned offsets.
// Double-precision library only (the float build has no double checker for delta): its entry points refuse.
// Front end, as every export's: whole_handle() and SP_REFUSE() (lbmdem_handle.h) for the refusals, OutFile (lbm_outfile.h) for
// the three files; the scratch is a call's own (a local MemPool), nothing is kept on the handle.
#include "lbm_device.h"
#include "lbm_outfile.h"

#include <type_traits>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

#ifndef LBMDEM_SINGLE_PRECISION
static_assert(sizeof(lbmdem_link) == 24, "lbmdem_link is the record the kernel stores");

// A workgroup owns LK_BX consecutive x by LK_BY consecutive y (64 x 64 nodes, 16 per lane).
//   in:      lanes run along y first -- obst[x][y] has y as the fast axis -- into LDS with a halo of 1: `act` of a node needs its
//            8 neighbours (act_rule's look at the lowest cover of a neighbour goes to the rasteriser's record in memory, not to
//            the map), a link its neighbour in direction q;
//   compute: lanes run along x first -- a wavefront holds one cell, the 64 consecutive x of one y, so that the order of the file
//            is the order of the lanes; the four wavefronts take every fourth y;
//   out:     act goes back through LDS and leaves with y as the fast axis; the records of a cell are consecutive.
// LDS banking (4-byte banks, 32 of them): the ids are read at (tx + 1) * LK_OPITCH + ty + 1 by lanes of consecutive tx --
// LK_OPITCH odd keeps them apart; the act bytes are written at tx * LK_APITCH + ty -- 17 words per tx, the same.
constexpr int LK_BX = 64, LK_BY = 64;
constexpr int LK_OX = LK_BX + 2, LK_OY = LK_BY + 2, LK_OPITCH = LK_OY + 1;
constexpr int LK_APITCH = LK_BY + 4;
static_assert(LK_BX == 64, "a cell is one wavefront");

struct LinksJob {
  const int* obst;       // the map of the most recent rasterisation, device layout [x][sy]
  LatticeView L;         // (the whole lattice: gx0 == 0, nxl == lx)
  GrainFluidView G;
  unsigned char* act;    // [lx][ly], or null
  long long* cells;      // count: [ly * nxb + 1] links per cell (zeroed beforehand), or null; emit: their exclusive scan
  unsigned long long* census;   // [6], count only
  lbmdem_link* out;      // emit only
  long long cap;         // records `out` holds
  int nxb;               // cells per y
};

// what one node contributes
struct NodeLinks {
  int act;          // the reference's act[x][y]
  int owner;        // the grain, -1 when the node takes no part
  unsigned mask;    // bit q: (P, q) is an effective link
  int resets;       // solid -> solid slots of an active node (the w[q] resets of main.c:1161, 1192)
};

template <int q, class Fn>
__device__ __forceinline__ void for_each_q(Fn&& fn) {
  fn(std::integral_constant<int, q>{});
  if constexpr (q < 8) for_each_q<q + 1>(fn);
}

__device__ __forceinline__ void stage_ids(const LinksJob& J, int* sO, int x0, int y0) {
  const LatticeView& L = J.L;
  for (int idx = threadIdx.x; idx < LK_OX * LK_OY; idx += 256) {
    const int ty = idx % LK_OY - 1, tx = idx / LK_OY - 1;
    const int gx = x0 + tx, gy = y0 + ty;
    int o = L.n;   // beyond the lattice: never looked at by an interior node
    if (gx >= 0 && gx < L.lx && gy >= 0 && gy < L.ly) o = J.obst[(long)gx * L.sy + gy];
    sO[(tx + 1) * LK_OPITCH + ty + 1] = o;
  }
}

__device__ __forceinline__ NodeLinks node_links(const LinksJob& J, const int* sO, int tx, int ty, int gx, int gy) {
  const LatticeView& L = J.L;
  auto ob = [&](int ex, int ey) { return sO[(tx + 1 + ex) * LK_OPITCH + ty + 1 + ey]; };
  NodeLinks r{0, -1, 0u, 0};
  // init_obst: act = 0 on the lattice-edge rows and columns (main.c:675-683); obst_construction: 1 on every interior node
  // (main.c:1000), then 0 or 1 on the nodes of a grain
  if (gx < 1 || gx > L.lx - 2 || gy < 1 || gy > L.ly - 2) return r;
  const int o = ob(0, 0);
  r.act = 1;
  if (o < 0 || o >= L.n) return r;
  r.owner = o;
  r.act = act_rule(L, J.G, ob, gx, gy) ? 1 : 0;
  if (!r.act) return r;
#pragma unroll
  for (int q = 1; q < 9; ++q) {
    if (ob(EXq(q), EYq(q)) == -1) r.mask |= 1u << q;
    else r.resets++;
  }
  return r;
}

__device__ __forceinline__ int wave_sum(int v) { return __builtin_amdgcn_readlane(wave_inclusive_scan(v), 63); }

__global__ __launch_bounds__(256) void k_links_count(const LinksJob J) {
  __shared__ int sO[LK_OX * LK_OPITCH];
  __shared__ unsigned char sA[LK_BX * LK_APITCH];
  __shared__ int sC[4][6];
  const LatticeView& L = J.L;
  const int x0 = blockIdx.x * LK_BX, y0 = blockIdx.y * LK_BY;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  stage_ids(J, sO, x0, y0);
  __syncthreads();
  int c[6] = {0, 0, 0, 0, 0, 0};
  for (int r = 0; r < LK_BY / 4; ++r) {   // (every lane of the wavefront stays in the loop: wave_sum moves data between lanes)
    const int tx = lane, ty = wave + 4 * r;
    const int gx = x0 + tx, gy = y0 + ty;
    const bool in = gx < L.lx && gy < L.ly;
    NodeLinks n{0, -1, 0u, 0};
    if (in) n = node_links(J, sO, tx, ty, gx, gy);
    sA[tx * LK_APITCH + ty] = (unsigned char)n.act;
    const int nl = __popc(n.mask);
    if (n.owner >= 0) {
      c[0]++; c[1] += n.act; c[2] += nl; c[5] += n.resets;
      if (n.mask) {
        const real xc = J.G.xc[n.owner], yc = J.G.yc[n.owner], r2 = J.G.r2[n.owner];
        for_each_q<1>([&](auto Q) {
          constexpr int q = decltype(Q)::value;
          if (n.mask >> q & 1u) {
            const real d = link_delta<q>(gx, gy, xc, yc, r2);
            if (d > 0. && d < 0.5) c[3]++;   // ibb_near
            if (d >= 0.5) c[4]++;            // ibb_far
          }
        });
      }
    }
    const int cell = wave_sum(nl);
    if (J.cells && lane == 0 && gy < L.ly) J.cells[(long)gy * J.nxb + blockIdx.x] = cell;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int s = wave_sum(c[k]);
    if (lane == 0) sC[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    atomicAdd(&J.census[k], (unsigned long long)(sC[0][k] + sC[1][k] + sC[2][k] + sC[3][k]));
  }
  if (J.act) {
    for (int idx = threadIdx.x; idx < LK_BX * LK_BY; idx += 256) {
      const int ty = idx % LK_BY, tx = idx / LK_BY;
      if (x0 + tx < L.lx && y0 + ty < L.ly) J.act[(size_t)(x0 + tx) * L.ly + y0 + ty] = sA[tx * LK_APITCH + ty];
    }
  }
}

__global__ __launch_bounds__(256) void k_links_emit(const LinksJob J) {
  __shared__ int sO[LK_OX * LK_OPITCH];
  const LatticeView& L = J.L;
  const int x0 = blockIdx.x * LK_BX, y0 = blockIdx.y * LK_BY;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  stage_ids(J, sO, x0, y0);
  __syncthreads();
  for (int r = 0; r < LK_BY / 4; ++r) {
    const int tx = lane, ty = wave + 4 * r;
    const int gx = x0 + tx, gy = y0 + ty;
    const bool in = gx < L.lx && gy < L.ly;
    NodeLinks n{0, -1, 0u, 0};
    if (in) n = node_links(J, sO, tx, ty, gx, gy);
    const int nl = __popc(n.mask);
    const int before = wave_inclusive_scan(nl) - nl;   // links of the cell's lower x
    if (n.mask) {
      long long at = J.cells[(long)gy * J.nxb + blockIdx.x] + before;
      const real xc = J.G.xc[n.owner], yc = J.G.yc[n.owner], r2 = J.G.r2[n.owner];
      for_each_q<1>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        if (n.mask >> q & 1u) {
          const real d = link_delta<q>(gx, gy, xc, yc, r2);
          // (a delta of exactly zero is a link the reference's file leaves out, main.c:1634: flagged by the sign of q)
          if (at < J.cap) J.out[at] = lbmdem_link{gx, gy, d != 0 ? q : -q, n.owner, (double)d};
          ++at;
        }
      });
    }
  }
}

// what the export describes: the map of the most recent rasterisation and the centres it was painted from
int geometry_job(lbmdem_handle* h, const char* who, LinksJob* J) {
  RC_TRY(whole_handle(h, who));
  const LatticeView& L = h->L;
  if (h->geo_buf < 0)
    return fail(LBMDEM_EINVAL, "%s: the centres of the last rasterisation are gone (the grains have moved on, or the map came from "
                               "a checkpoint): the export describes a map again after the next lbmdem_obst_construction or fluid step", who);
  *J = LinksJob{};
  J->obst = h->obst[h->geo_buf];
  J->L = L;
  J->L.gate = nullptr;
  J->G = gview(h);
  J->nxb = (L.lx + LK_BX - 1) / LK_BX;
  return LBMDEM_OK;
}

dim3 links_grid(const LinksJob& J) { return dim3(J.nxb, (J.L.ly + LK_BY - 1) / LK_BY); }

// pass 1 into act_dev ([lx][ly] bytes, may be null), cells (J.cells, may be null) and census6_dev
int links_count(lbmdem_handle* h, LinksJob J, unsigned char* act_dev, unsigned long long* census_dev) {
  J.act = act_dev;
  J.census = census_dev;
  HIP_TRY(hipMemsetAsync(census_dev, 0, 6 * sizeof(unsigned long long), h->stream));
  if (J.cells) HIP_TRY(hipMemsetAsync(J.cells, 0, sizeof(long long) * ((size_t)J.L.ly * J.nxb + 1), h->stream));
  hipLaunchKernelGGL(k_links_count, links_grid(J), dim3(256), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

int put_map(const char* dir, const char* name, int lx, int ly, const int* a) {
  OutFile F;
  RC_TRY(F.open("w", dir, "%s", name));
  for (int y = 0; y < ly; y++) {   // main.c:1606-1612, 1619-1624
    for (int x = 0; x < lx; x++) fprintf(F.fp, "%d ", a[(size_t)x * ly + y]);
    fprintf(F.fp, "\n");
  }
  return F.close();
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_obst_files(const char* dir, int lx, int ly, const int* obst, const int* act, const lbmdem_link* links, long n) {
  if (!obst || !act || (n > 0 && !links) || n < 0 || lx < 1 || ly < 1) return fail(LBMDEM_EINVAL, "bad lbmdem_write_obst_files arguments");
  RC_TRY(put_map(dir, "obst_LB.dat", lx, ly, obst));
  RC_TRY(put_map(dir, "active_nodes.dat", lx, ly, act));
  OutFile F;
  RC_TRY(F.open("w", dir, "links.dat"));
  for (long k = 0; k < n; k++)   // main.c:1631-1639; the list is in that order already
    if (links[k].delta != 0) fprintf(F.fp, "%d  %d  %d  %f\n", links[k].x, links[k].y, links[k].q < 0 ? -links[k].q : links[k].q, links[k].delta);
  return F.close();
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_geometry_stats(lbmdem_handle* h, long*) { SP_REFUSE(h, "the boundary-link export"); }
int lbmdem_download_act(lbmdem_handle* h, int*) { SP_REFUSE(h, "the boundary-link export"); }
int lbmdem_download_links(lbmdem_handle* h, lbmdem_link*, long, long*) { SP_REFUSE(h, "the boundary-link export"); }
int lbmdem_download_geometry_obst(lbmdem_handle* h, int*) { SP_REFUSE(h, "the boundary-link export"); }
int lbmdem_write_obst(lbmdem_handle* h, const char*) { SP_REFUSE(h, "the boundary-link export"); }
#else

int lbmdem_geometry_stats(lbmdem_handle* h, long* counts6) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts6) return fail(LBMDEM_EINVAL, "null buffer");
  LinksJob J;
  RC_TRY(geometry_job(h, "lbmdem_geometry_stats", &J));
  MemPool scratch;   // (device memory of this call)
  unsigned long long* census = nullptr;
  HIP_TRY(scratch.dev(&census, 6));
  RC_TRY(links_count(h, J, nullptr, census));
  unsigned long long c[6];
  HIP_TRY(hipMemcpyAsync(c, census, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 6; ++k) counts6[k] = (long)c[k];
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_act(lbmdem_handle* h, int* act) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!act) return fail(LBMDEM_EINVAL, "null buffer");
  LinksJob J;
  RC_TRY(geometry_job(h, "lbmdem_download_act", &J));
  const size_t nodes = (size_t)J.L.lx * J.L.ly;
  MemPool scratch;
  unsigned long long* census = nullptr;
  unsigned char* bytes = nullptr;
  HIP_TRY(scratch.dev(&census, 6));
  HIP_TRY(scratch.dev(&bytes, nodes));
  RC_TRY(links_count(h, J, bytes, census));
  std::vector<unsigned char> host(nodes);
  HIP_TRY(hipMemcpyAsync(host.data(), bytes, nodes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < nodes; ++k) act[k] = host[k];
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_links(lbmdem_handle* h, lbmdem_link* out, long cap, long* count) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!count || (cap > 0 && !out) || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  LinksJob J;
  RC_TRY(geometry_job(h, "lbmdem_download_links", &J));
  const size_t ncell = (size_t)J.L.ly * J.nxb;
  MemPool scratch;
  unsigned long long* census = nullptr;
  long long *cells = nullptr, *offsets = nullptr;
  void* tmp = nullptr;
  lbmdem_link* links = nullptr;
  HIP_TRY(scratch.dev(&census, 6));
  HIP_TRY(scratch.dev(&cells, ncell + 1));
  HIP_TRY(scratch.dev(&offsets, ncell + 1));
  J.cells = cells;
  RC_TRY(links_count(h, J, nullptr, census));
  // the cells in file order, one empty cell behind the last: its offset is the number of links
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cells, offsets, (int)(ncell + 1), h->stream));
  HIP_TRY(scratch.dev(&tmp, tmp_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cells, offsets, (int)(ncell + 1), h->stream));
  long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, offsets + ncell, sizeof total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *count = (long)total;
  if (cap == 0) return LBMDEM_OK;   // (how many there are)
  if (cap < total) return fail(LBMDEM_EINVAL, "lbmdem_download_links: there are %lld links, the buffer holds %ld", total, cap);
  if (total == 0) return LBMDEM_OK;
  HIP_TRY(scratch.dev(&links, (size_t)total));
  J.cells = offsets;
  J.out = links;
  J.cap = total;
  hipLaunchKernelGGL(k_links_emit, links_grid(J), dim3(256), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, links, sizeof(lbmdem_link) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_geometry_obst(lbmdem_handle* h, int* obst) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!obst) return fail(LBMDEM_EINVAL, "null buffer");
  LinksJob J;
  RC_TRY(geometry_job(h, "lbmdem_download_geometry_obst", &J));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy2D(obst, sizeof(int) * J.L.ly, J.obst, sizeof(int) * J.L.sy, sizeof(int) * J.L.ly, J.L.lx, hipMemcpyDeviceToHost));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_obst(lbmdem_handle* h, const char* dir) try {
  CHECK_H(h);
  const size_t nodes = (size_t)h->L.lx * h->L.ly;
  std::vector<int> obst(nodes), act(nodes);
  RC_TRY(lbmdem_download_geometry_obst(h, obst.data()));
  RC_TRY(lbmdem_download_act(h, act.data()));
  long n = 0;
  RC_TRY(lbmdem_download_links(h, nullptr, 0, &n));
  std::vector<lbmdem_link> links((size_t)(n > 0 ? n : 1));
  if (n > 0) RC_TRY(lbmdem_download_links(h, links.data(), n, &n));
  return lbmdem_write_obst_files(dir, h->L.lx, h->L.ly, obst.data(), act.data(), links.data(), n);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
