// lbm_scalar.hip -- the passive scalar (lbmdem_scalar_set, lbmdem_scalar_step, lbmdem_scalar_download, lbmdem_scalar_download_state,
// lbmdem_scalar_device, lbmdem_scalar_sums, lbmdem_scalar_stats, lbmdem_write_scalar, lbmdem_write_scalar_files,
// lbmdem_set_scalar_output; include/lbmdem_hip.h): a dye field carried by the fluid's velocity and diffused, a second lattice of
// five populations per node (rest and the four axis directions) stepped once per fluid step, on the device. The reference has no
// such routine: the contract is the arithmetic the header spells out, every expression associated as written there.
//
//   k_scalar_refill  the pre-pass, one lane per node, lanes along y: a fluid node the scalar did not hold (a grain has uncovered
//                    it) takes w_k times the mean concentration of its axis neighbours that are fluid and were held. In place:
//                    it reads only nodes inside was_fluid and writes only nodes outside it, so nothing races.
//   k_scalar_step    a workgroup owns a window of 256 columns (lanes along y, the contiguous axis of f, obst and the planes of g)
//                    and a segment of SC_SEG lattice rows, and marches along x as k_flow_nodes does: a node's velocity
//                    (node_vel, lbm_device.h: the flow fields' and the tracers' formulas) and its five post-collision values
//                    are formed ONCE and handed on -- x -+ 1 through the rows kept in registers, y -+ 1 through the neighbouring
//                    lanes (wave shifts; the first and the last lane of a wave form one halo column each). It reads buffer
//                    `cur` and writes the other one (ping-pong), and was_fluid, which nothing in this launch reads.
//   k_scalar_init    lbmdem_scalar_set: g_k = w_k * C on the fluid nodes, +0.0 elsewhere, was_fluid.
//   k_scalar_conc    the concentration plane [lx][ly] for the download, the torch view and the file.
//   k_scalar_blocks, k_scalar_rows, k_scalar_total   the sums, chains in the flow sums' order (64 y, a row's blocks, the rows).
// g is five planes [k][lx][sy] at the map's row pitch (sy, a multiple of 16): a wave's row is 512 contiguous, 128-byte aligned
// bytes per plane. No atomics, no LDS on the step path, nothing depends on launch order. Both step kernels are gated: queued behind
// a launch of k_dem_chain that gave up they do nothing, and the replay makes the step again.
// With no scalar set nothing is allocated or launched. Double-precision library only: the entry points that take a handle refuse
// in the float build; the host-only file writer exists in both.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h), MemPool (lbm_mem.h) for the
// buffers kept on the handle, OutFile (lbm_outfile.h) for the file.
#include "lbm_device.h"
#include "lbm_outfile.h"

namespace {

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int SC_SUMS = 5;        // n_fluid, sum C, sum C * C, min C, max C
constexpr int SC_K = 5;          // populations per node: q = 0, 2, 4, 6, 8 of the fluid's set
constexpr int SC_THREADS = 256;   // columns of a window
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_SEG = 32;        // rows of a segment
constexpr int SC_BLOCK = 64;      // y per sum block: one wave
constexpr int SC_CHAINS = 4;      // per (row, block): sum C, sum C * C, min C, max C
constexpr int SC_PITCH = SC_BLOCK + 2;   // (k_flow_nodes' pitch: the serial lanes start 4 banks apart)
constexpr double SC_W0 = 1. / 3, SC_W1 = 1. / 6;

struct ScalarJob {
  const real* f;
  const int* obst;       // device layout [x][sy]
  LatticeView L;         // (the whole lattice: gx0 == 0, nxl == lx)
  Kin K;
  double* gin;           // [5][lx][sy]: the stored populations (the pre-pass refills them in place)
  double* gout;          // the other buffer
  unsigned char* was;    // [lx][sy]
  long plane;            // lx * sy
  double omega;
};

// C of the header: the stored populations of node `at`, added left to right
__device__ __forceinline__ double sc_conc(const double* __restrict__ g, long plane, long at) {
  return g[at] + g[plane + at] + g[2 * plane + at] + g[3 * plane + at] + g[4 * plane + at];
}

__global__ __launch_bounds__(SC_THREADS) void k_scalar_refill(const ScalarJob J) {
  LBMDEM_GATE(J.L.gate);
  const LatticeView& L = J.L;
  const int y = blockIdx.x * SC_THREADS + threadIdx.x, x = blockIdx.y;
  if (y >= L.ly) return;
  const long at = (long)x * L.sy + y;
  if (J.obst[at] != -1 || J.was[at]) return;
  double s = 0.;
  int cnt = 0;
#pragma unroll
  for (int q = 2; q <= 8; q += 2) {   // the axis neighbours in the order q = 2, 4, 6, 8
    const int xn = x + EXq(q), yn = y + EYq(q);
    if (xn < 0 || xn >= L.lx || yn < 0 || yn >= L.ly) continue;
    const long an = (long)xn * L.sy + yn;
    if (J.obst[an] != -1 || !J.was[an]) continue;
    s = s + sc_conc(J.gin, J.plane, an);
    ++cnt;
  }
  const double Cf = cnt ? s / (double)cnt : 0.;
  J.gin[at] = SC_W0 * Cf;
#pragma unroll
  for (int k = 1; k < SC_K; ++k) J.gin[k * J.plane + at] = SC_W1 * Cf;
}

// the five post-collision values of node (x, y) and whether it is fluid; +0.0 and 0 where it is not
__device__ __forceinline__ void sc_collide(const ScalarJob& J, int x, int y, double (&gs)[SC_K], int& fl) {
  const LatticeView& L = J.L;
  const long at = (long)x * L.sy + y;
  const int o = J.obst[at];
#pragma unroll
  for (int k = 0; k < SC_K; ++k) gs[k] = 0.;
  fl = 0;
  if (o != -1) return;
  real f[9];
  const NodeVel N = node_vel(J.f, o, L, J.K, x, y, f);   // (lbm_device.h: shared with the flow fields and the tracers)
  double g[SC_K];
#pragma unroll
  for (int k = 0; k < SC_K; ++k) g[k] = J.gin[k * J.plane + at];
  const double C = g[0] + g[1] + g[2] + g[3] + g[4];
  const double a0 = SC_W0 * C, a = SC_W1 * C;
  // e_k . u for k = 1..4 (q = 2, 4, 6, 8): -ux, -uy, ux, uy; for k = 0 the bracket is 1. exactly
  const double eq[SC_K] = {a0, a * (1. + 3. * (-N.ux)), a * (1. + 3. * (-N.uy)), a * (1. + 3. * N.ux), a * (1. + 3. * N.uy)};
#pragma unroll
  for (int k = 0; k < SC_K; ++k) gs[k] = g[k] - J.omega * (g[k] - eq[k]);
  fl = 1;
}

// a lattice row as the march keeps it: the lane's node and what its two neighbours in y send towards it
struct ScRow { double g[SC_K], gm, gp; int fl, flm, flp; };

__global__ __launch_bounds__(SC_THREADS) void k_scalar_step(const ScalarJob J) {
  LBMDEM_GATE(J.L.gate);
  const LatticeView& L = J.L;
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * SC_THREADS + threadIdx.x;
  const int xa = blockIdx.y * SC_SEG;
  const int xb = xa + SC_SEG < L.lx ? xa + SC_SEG : L.lx;
  const bool in = y < L.ly;
  const int yh = lane == 0 ? y - 1 : y + 1;   // the halo column of a wave's first and last lane
  const bool halo = (lane == 0 || lane == 63) && yh >= 0 && yh < L.ly;
  ScRow cur{};
  double prev3 = 0.;   // of row xc - 1: what it sends along +x, and whether it is fluid
  int prevfl = 0;
  for (int xr = xa - 1; xr <= xb; ++xr) {   // (every lane stays in the loop: wave shifts)
    ScRow nx{};
    if (xr >= 0 && xr < L.lx) {
      int fl = 0;
      double gs[SC_K] = {0., 0., 0., 0., 0.};
      if (in) sc_collide(J, xr, y, gs, fl);
      double hg = 0.;
      int hfl = 0;
      if (halo && xr >= xa && xr < xb) {   // (the rows in front of and behind the segment only send along x)
        double hs[SC_K];
        sc_collide(J, xr, yh, hs, hfl);
        hg = lane == 0 ? hs[4] : hs[2];
      }
#pragma unroll
      for (int k = 0; k < SC_K; ++k) nx.g[k] = gs[k];
      nx.fl = fl;
      nx.gm = __shfl_up(gs[4], 1); nx.flm = __shfl_up(fl, 1);       // from (x, y - 1), moving along +y
      nx.gp = __shfl_down(gs[2], 1); nx.flp = __shfl_down(fl, 1);   // from (x, y + 1), moving along -y
      if (lane == 0) { nx.gm = hg; nx.flm = hfl; }
      if (lane == 63) { nx.gp = hg; nx.flp = hfl; }
    }
    const int xc = xr - 1;   // `cur` is row xc: with `prev` and `nx` around it, it is complete
    if (xc >= xa && in) {    // (xc < xb: xr <= xb)
      const long at = (long)xc * L.sy + y;
      double o[SC_K] = {0., 0., 0., 0., 0.};
      if (cur.fl) {          // the pull: from the node behind where that is fluid, else the node's own opposite value
        o[0] = cur.g[0];
        o[1] = nx.fl ? nx.g[1] : cur.g[3];      // e_1 = (-1, 0): from (xc + 1, y)
        o[2] = cur.flp ? cur.gp : cur.g[4];     // e_2 = (0, -1): from (xc, y + 1)
        o[3] = prevfl ? prev3 : cur.g[1];       // e_3 = (1, 0): from (xc - 1, y)
        o[4] = cur.flm ? cur.gm : cur.g[2];     // e_4 = (0, 1): from (xc, y - 1)
      }
#pragma unroll
      for (int k = 0; k < SC_K; ++k) J.gout[k * J.plane + at] = o[k];
      J.was[at] = (unsigned char)cur.fl;
    }
    prev3 = cur.g[3];
    prevfl = cur.fl;
    cur = nx;
  }
}

// lbmdem_scalar_set: C is [lx][ly] as the host gave it
__global__ __launch_bounds__(SC_THREADS) void k_scalar_init(const double* __restrict__ C, const int* __restrict__ obst, int lx, int ly,
                                                            int sy, long plane, double* __restrict__ g, unsigned char* __restrict__ was) {
  const int y = blockIdx.x * SC_THREADS + threadIdx.x, x = blockIdx.y;
  if (y >= ly) return;
  const long at = (long)x * sy + y;
  const bool fl = obst[at] == -1;
  const double c = fl ? C[(long)x * ly + y] : 0.;
  g[at] = fl ? SC_W0 * c : 0.;
#pragma unroll
  for (int k = 1; k < SC_K; ++k) g[k * plane + at] = fl ? SC_W1 * c : 0.;
  was[at] = fl;
}

// the concentration plane [lx][ly]: a node outside was_fluid holds five +0.0
__global__ __launch_bounds__(SC_THREADS) void k_scalar_conc(const double* __restrict__ g, int ly, int sy, long plane,
                                                            double* __restrict__ C) {
  const int y = blockIdx.x * SC_THREADS + threadIdx.x, x = blockIdx.y;
  if (y >= ly) return;
  C[(long)x * ly + y] = sc_conc(g, plane, (long)x * sy + y);
}

// the sums' chains: k = 0 the count, 1 and 2 sums from +0.0, 3 the minimum from +inf, 4 the maximum from -inf
__device__ __forceinline__ double sc_start(int k) { return k < 3 ? 0. : (k == 3 ? (double)INFINITY : -(double)INFINITY); }
__device__ __forceinline__ double sc_fold(int k, double a, double v) { return k < 3 ? a + v : (k == 3 ? fmin(a, v) : fmax(a, v)); }

// part[x][b][5]: per row and block of 64 y (one wave) the count and the four chains over y ascending; a node outside was_fluid
// adds +0.0 and does not enter the minimum or the maximum
__global__ __launch_bounds__(SC_THREADS) void k_scalar_blocks(const double* __restrict__ g, const unsigned char* __restrict__ was,
                                                              int ly, int sy, long plane, int nb, double* __restrict__ part) {
  __shared__ double sS[SC_WAVES][SC_CHAINS][SC_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.x * SC_THREADS + threadIdx.x, x = blockIdx.y;
  bool fl = false;
  double C = 0.;
  if (y < ly) {
    const long at = (long)x * sy + y;
    fl = was[at] != 0;
    if (fl) C = sc_conc(g, plane, at);
  }
  sS[wave][0][lane] = fl ? C : 0.;
  sS[wave][1][lane] = fl ? C * C : 0.;
  sS[wave][2][lane] = fl ? C : sc_start(3);
  sS[wave][3][lane] = fl ? C : sc_start(4);
  const unsigned long long fluid_lanes = __ballot(fl);
  __syncthreads();
  const int yw = y - lane;   // the block's first column
  if (yw < ly && lane < SC_SUMS) {
    double a = (double)__popcll(fluid_lanes);
    if (lane > 0) {
      a = sc_start(lane);
      const double* s = sS[wave][lane - 1];
      for (int k = 0; k < SC_BLOCK; ++k) a = sc_fold(lane, a, s[k]);
    }
    part[((long)x * nb + yw / SC_BLOCK) * SC_SUMS + lane] = a;
  }
}

// rows[x][k]: the chain of row x's block values, blocks ascending
__global__ __launch_bounds__(256) void k_scalar_rows(const double* __restrict__ part, int lx, int nb, double* __restrict__ rows) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)lx * SC_SUMS) return;
  const int k = (int)(id % SC_SUMS);
  const double* p = part + (id / SC_SUMS) * nb * SC_SUMS + k;
  double a = sc_start(k);
  for (int b = 0; b < nb; ++b) a = sc_fold(k, a, p[(long)b * SC_SUMS]);
  rows[id] = a;
}

// sums[k]: the chain of the row values over x ascending. One workgroup: 256 rows at a time through LDS, five lanes fold serially.
__global__ __launch_bounds__(256) void k_scalar_total(const double* __restrict__ rows, int lx, double* __restrict__ sums) {
  __shared__ double sR[256 * SC_SUMS];
  const int t = threadIdx.x;
  double a = sc_start(t < SC_SUMS ? t : 0);
  for (int x0 = 0; x0 < lx; x0 += 256) {
    const int nr = lx - x0 < 256 ? lx - x0 : 256;
    for (int e = t; e < nr * SC_SUMS; e += 256) sR[e] = rows[(long)x0 * SC_SUMS + e];
    __syncthreads();
    if (t < SC_SUMS)
      for (int r = 0; r < nr; ++r) a = sc_fold(t, a, sR[r * SC_SUMS + t]);
    __syncthreads();
  }
  if (t < SC_SUMS) sums[t] = a;
}

dim3 sc_node_grid(const LatticeView& L) { return dim3((L.ly + SC_THREADS - 1) / SC_THREADS, L.lx); }

// the scalar gone and its buffers given back now, not when the handle ends
void scalar_free(lbmdem_handle* h) {
  ScalarState& S = h->scalar;
  h->mem.release(S.g[0]);
  h->mem.release(S.g[1]);
  h->mem.release(S.was);
  h->mem.release(S.conc);
  h->mem.release(S.part);
  h->mem.release(S.sums);
  S = ScalarState{};
}

// the concentration plane of the present state into S.conc, on the handle's stream
int scalar_conc_launch(lbmdem_handle* h) {
  const ScalarState& S = h->scalar;
  const LatticeView& L = h->L;
  hipLaunchKernelGGL(k_scalar_conc, sc_node_grid(L), dim3(SC_THREADS), 0, h->stream, S.g[S.cur], L.ly, L.sy, (long)L.lx * L.sy,
                     S.conc);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}

int scalar_sums_now(lbmdem_handle* h, double* out5) {
  ScalarState& S = h->scalar;
  const LatticeView& L = h->L;
  const int nb = (L.ly + SC_BLOCK - 1) / SC_BLOCK;
  HIP_TRY(h->mem.grow(&S.part, &S.part_cap, (long)L.lx * nb * SC_SUMS + (long)L.lx * SC_SUMS));
  if (!S.sums) HIP_TRY(h->mem.dev(&S.sums, (size_t)SC_SUMS));
  double* rows = S.part + (long)L.lx * nb * SC_SUMS;
  hipLaunchKernelGGL(k_scalar_blocks, sc_node_grid(L), dim3(SC_THREADS), 0, h->stream, S.g[S.cur], S.was, L.ly, L.sy,
                     (long)L.lx * L.sy, nb, S.part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_scalar_rows, dim3((unsigned)(((long)L.lx * SC_SUMS + 255) / 256)), dim3(256), 0, h->stream, S.part, L.lx, nb,
                     rows);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_scalar_total, dim3(1), dim3(256), 0, h->stream, rows, L.lx, S.sums);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out5, S.sums, sizeof(double) * SC_SUMS, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (out5[0] == 0.) out5[3] = out5[4] = 0.;   // no fluid node: the extremes read +0.0
  return LBMDEM_OK;
}

#define SCALAR_SET(h, who) do { if (!(h)->scalar.on) return fail(LBMDEM_EINVAL, who ": no scalar is set (lbmdem_scalar_set first)"); } while (0)
#endif   // !LBMDEM_SINGLE_PRECISION

inline unsigned be_float(double v) {
  const float f = (float)v;
  unsigned u;
  memcpy(&u, &f, 4);
  return __builtin_bswap32(u);
}

// scalar%.6i.vtk: legacy binary STRUCTURED_POINTS on the nodes of the frames' mesh, (float)C, x fastest
int scalar_write_file(const char* dir, int nfile, int lx, int ly, const double* C) {
  const size_t cnt = (size_t)lx * ly;
  std::vector<unsigned> image(cnt);
  for (int y = 0; y < ly; ++y)
    for (int x = 0; x < lx; ++x) image[(size_t)y * lx + x] = be_float(C[(size_t)x * ly + y]);
  const float pas = (float)(1. / lx);   // (lbmdem_vtk_put_mesh's)
  OutFile F;
  RC_TRY(F.open("w+", dir, "scalar%.6i.vtk", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# vtk DataFile Version 2.0\nlbmdem passive scalar\nBINARY\nDATASET STRUCTURED_POINTS\n");
  fprintf(fp, "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\n", lx, ly, (double)pas, (double)pas);
  fprintf(fp, "POINT_DATA %zu\nSCALARS concentration float\nLOOKUP_TABLE default\n", cnt);
  const bool short_write = fwrite(image.data(), 4, cnt, fp) != cnt;
  return F.close(short_write);
}

}  // namespace

int lbmdem_scalar_launch(lbmdem_handle* h, const int* obst, bool hook) {
#ifdef LBMDEM_SINGLE_PRECISION
  (void)h; (void)obst; (void)hook;
  return fail(LBMDEM_EINVAL, "the passive scalar is not available in the single-precision build of the library");
#else
  ScalarState& S = h->scalar;
  if (!S.on) return LBMDEM_OK;
  const LatticeView& L = h->L;
  ScalarJob J{};
  J.f = h->f[h->fcur];
  J.obst = obst;
  J.L = L;
  J.K = h->kin[h->kcur];
  J.gin = S.g[S.cur];
  J.gout = S.g[1 - S.cur];
  J.was = S.was;
  J.plane = (long)L.lx * L.sy;
  J.omega = S.omega;
  hipLaunchKernelGGL(k_scalar_refill, sc_node_grid(L), dim3(SC_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_scalar_step, dim3((L.ly + SC_THREADS - 1) / SC_THREADS, (L.lx + SC_SEG - 1) / SC_SEG), dim3(SC_THREADS), 0,
                     h->stream, J);
  HIP_TRY(hipGetLastError());
  S.cur = 1 - S.cur;
  S.steps++;
  if (hook) S.hook++;
  return LBMDEM_OK;
#endif
}

int lbmdem_scalar_data_line(lbmdem_handle* h, const char* dir) {
#ifdef LBMDEM_SINGLE_PRECISION
  (void)h; (void)dir;
  return fail(LBMDEM_EINVAL, "the passive scalar is not available in the single-precision build of the library");
#else
  double s[SC_SUMS];
  RC_TRY(lbmdem_scalar_sums(h, s));
  OutFile F;
  RC_TRY(F.open("a", dir, "scalar.data"));
  FILE* fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0) fprintf(fp, "# step n_fluid sum_C sum_C2 min_C max_C\n");
  fprintf(fp, "%le", (double)h->nbsteps);
  for (int k = 0; k < SC_SUMS; ++k) fprintf(fp, " %le", s[k]);
  fprintf(fp, "\n");
  return F.close(false);
#endif
}

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_scalar_files(const char* dir, int nfile, int lx, int ly, const double* C) try {
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  if (!C) return fail(LBMDEM_EINVAL, "null buffer");
  if (lx < 2 || ly < 2) return fail(LBMDEM_EINVAL, "lbmdem_write_scalar_files: the lattice is %d x %d", lx, ly);
  return scalar_write_file(dir, nfile, lx, ly, C);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_scalar_set(lbmdem_handle* h, const double*, double, int) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_scalar_step(lbmdem_handle* h) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_scalar_download(lbmdem_handle* h, double*) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_scalar_download_state(lbmdem_handle* h, double*, unsigned char*) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_scalar_device(lbmdem_handle* h, void**, int) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_scalar_sums(lbmdem_handle* h, double*) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_scalar_stats(lbmdem_handle* h, long*) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_write_scalar(lbmdem_handle* h, const char*, int) { SP_REFUSE(h, "the passive scalar"); }
int lbmdem_set_scalar_output(lbmdem_handle* h, int) { SP_REFUSE(h, "the passive scalar"); }
#else

int lbmdem_scalar_set(lbmdem_handle* h, const double* C, double tau_s, int automatic) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_scalar_set"));
  const LatticeView& L = h->L;
  const long cnt = (long)L.lx * L.ly, plane = (long)L.lx * L.sy;
  if (C) {
    if (!(tau_s > 0.5) || !isfinite(tau_s))
      return fail(LBMDEM_EINVAL, "lbmdem_scalar_set: the relaxation time must be finite and larger than 0.5 (tau_s = %.17g)", tau_s);
    for (long k = 0; k < cnt; ++k)
      if (!isfinite(C[k]))
        return fail(LBMDEM_EINVAL, "lbmdem_scalar_set: C[%ld][%ld] = %g is not finite", k / L.ly, k % L.ly, C[k]);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));   // (a step of the earlier scalar may be in flight)
  scalar_free(h);
  if (!C) return LBMDEM_OK;
  ScalarState S{};
  if (h->mem.dev(&S.g[0], (size_t)(SC_K * plane)) != hipSuccess || h->mem.dev(&S.g[1], (size_t)(SC_K * plane)) != hipSuccess ||
      h->mem.dev(&S.was, (size_t)plane) != hipSuccess || h->mem.dev(&S.conc, (size_t)cnt) != hipSuccess) {
    h->mem.release(S.g[0]); h->mem.release(S.g[1]); h->mem.release(S.was); h->mem.release(S.conc);
    return fail(LBMDEM_ENOMEM, "lbmdem_scalar_set: device allocation of %zu bytes failed",
                2 * SC_K * sizeof(double) * (size_t)plane + (size_t)plane + sizeof(double) * (size_t)cnt);
  }
  S.on = true;
  S.automatic = automatic != 0;
  S.tau = tau_s;
  S.omega = 1. / tau_s;
  h->scalar = S;   // (from here on scalar_free gives everything back)
  // the padding columns (y >= ly) are written by no kernel: zero, so that the sections of a checkpoint that carries the scalar
  // (lbmdem_set_checkpoint_contents) do not depend on what the allocations held before
  hipError_t e = hipMemsetAsync(S.g[0], 0, sizeof(double) * (size_t)(SC_K * plane), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S.g[1], 0, sizeof(double) * (size_t)(SC_K * plane), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S.was, 0, (size_t)plane, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(S.conc, C, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_scalar_init, sc_node_grid(L), dim3(SC_THREADS), 0, h->stream, S.conc, reader_obst(h), L.lx, L.ly, L.sy, plane,
                       S.g[0], S.was);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    scalar_free(h);
    return fail(LBMDEM_EHIP, "lbmdem_scalar_set: setting the field on the device failed: %s", hipGetErrorString(e));
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_scalar_step(lbmdem_handle* h) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_scalar_step"));
  return lbmdem_scalar_launch(h, reader_obst(h), false);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_scalar_download(lbmdem_handle* h, double* C) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_scalar_download"));
  if (!C) return fail(LBMDEM_EINVAL, "null buffer");
  SCALAR_SET(h, "lbmdem_scalar_download");
  RC_TRY(scalar_conc_launch(h));
  HIP_TRY(hipMemcpyAsync(C, h->scalar.conc, sizeof(double) * (size_t)h->L.lx * h->L.ly, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_scalar_download_state(lbmdem_handle* h, double* g, unsigned char* was) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_scalar_download_state"));
  if (!g || !was) return fail(LBMDEM_EINVAL, "null buffer");
  SCALAR_SET(h, "lbmdem_scalar_download_state");
  const ScalarState& S = h->scalar;
  const LatticeView& L = h->L;
  const size_t plane = (size_t)L.lx * L.sy;
  std::vector<double> gd(SC_K * plane);
  std::vector<unsigned char> wd(plane);
  HIP_TRY(hipMemcpyAsync(gd.data(), S.g[S.cur], sizeof(double) * gd.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(wd.data(), S.was, wd.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int x = 0; x < L.lx; ++x)
    for (int y = 0; y < L.ly; ++y) {
      const size_t at = (size_t)x * L.sy + y, o = (size_t)x * L.ly + y;
      for (int k = 0; k < SC_K; ++k) g[SC_K * o + k] = gd[k * plane + at];
      was[o] = wd[at];
    }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_scalar_device(lbmdem_handle* h, void** C, int refresh) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_scalar_device"));
  if (!C) return fail(LBMDEM_EINVAL, "null argument");
  *C = h->scalar.conc;   // (null while no scalar is set)
  if (refresh && h->scalar.on) RC_TRY(scalar_conc_launch(h));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_scalar_sums(lbmdem_handle* h, double* out5) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_scalar_sums"));
  if (!out5) return fail(LBMDEM_EINVAL, "null buffer");
  SCALAR_SET(h, "lbmdem_scalar_sums");
  return scalar_sums_now(h, out5);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_scalar_stats(lbmdem_handle* h, long* counts3) try {
  CHECK_H(h);   // (settles: the counts are those of the steps that took place)
  RC_TRY(whole_handle(h, "lbmdem_scalar_stats"));
  if (!counts3) return fail(LBMDEM_EINVAL, "null argument");
  counts3[0] = h->scalar.on ? 1 : 0; counts3[1] = h->scalar.steps; counts3[2] = h->scalar.hook;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_scalar(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_write_scalar"));
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  SCALAR_SET(h, "lbmdem_write_scalar");
  std::vector<double> C((size_t)h->L.lx * h->L.ly);
  RC_TRY(scalar_conc_launch(h));
  HIP_TRY(hipMemcpyAsync(C.data(), h->scalar.conc, sizeof(double) * C.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return scalar_write_file(dir, nfile, h->L.lx, h->L.ly, C.data());
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_scalar_output(lbmdem_handle* h, int on) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) RC_TRY(whole_handle(h, "lbmdem_set_scalar_output"));
  h->scalar_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
