// lbm_flow.hip -- flow fields (lbmdem_flow_fields, lbmdem_flow_fields_device, lbmdem_flow_sums, lbmdem_write_flow,
// lbmdem_write_flow_files, lbmdem_set_flow_output; include/lbmdem_hip.h): the composite velocity of fluid and grains as the
// reference's velocity_profile mixes it (main.c:1659-1672), its vorticity and divergence, the non-equilibrium stress moments the
// MRT collision forms and throws away (main.c:1095-1106) with the strain rate, shear rate and dissipation that follow from them,
// and the fluid's sums. The reference has no such routine: the contract is the arithmetic the header spells out, every expression
// associated as written there. Nothing here is on the step path: the kernels only read the handle's state.
//
//   k_flow_nodes  a workgroup owns a window of 256 columns (lanes along y, the contiguous axis of f[x][y / 16][q][y % 16] and
//                 obst[x][y]) and a segment of FL_SEG lattice rows, and marches along x with the composite velocity of rows
//                 x - 1, x, x + 1 in registers; y -+ 1 comes from the neighbouring lanes (wave shifts), the first and the last
//                 lane of a wave read one halo column each. f and obst of a node are read once per segment (plus the two rows in
//                 front of and behind it); no velocity lattice exists in memory. It writes the selected planes, coalesced along y,
//                 and -- when sums are asked for -- per (row, block of 64 y = one wave) the chains over y: the addends go to LDS,
//                 seven lanes add or maximise serially;
//   k_flow_rows   per row the chain of its block sums, blocks ascending;
//   k_flow_total  one workgroup: the chain of the row sums over x ascending;
//   k_flow_image  planes -> the payloads of flow%.6i.vtk in file byte order (x fastest, big-endian float), a transpose through
//                 LDS as k_vtk_frame's.
// No atomics, nothing depends on launch order. Double-precision library only: the entry points that take a handle refuse in the
// float build; the host-only file writer exists in both.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h) for the refusals and the map,
// MemPool::grow (lbm_mem.h) for the scratch kept on the handle, OutFile (lbm_outfile.h) for the file.
#include "lbm_device.h"
#include "lbm_outfile.h"

#include <errno.h>

namespace {

constexpr int FL_FIELDS = 8;    // bits of the mask: ux uy vort div nxx nxy gdot diss
constexpr int FL_SUMS = 8;      // n_fluid, four sums, three maxima
constexpr int FL_FILE_WORDS = 6;   // floats per node in the file: the vector's three, three scalars

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int FL_THREADS = 256;   // columns of a window
constexpr int FL_WAVES = FL_THREADS / 64;
constexpr int FL_SEG = 32;        // rows of a segment
constexpr int FL_BLOCK = 64;      // y per sum block: one wave
constexpr int FL_CHAINS = 7;      // per (row, block): sum rho, ke, diss, enstrophy; max u2, gdot, |div|
// LDS: a chain's 64 addends at a pitch of 66 doubles = 132 words -- the seven serial lanes start 4 banks apart
constexpr int FL_PITCH = FL_BLOCK + 2;

struct FlowJob {
  const real* f;
  const int* obst;       // the map the last fluid step saw, device layout [x][sy]
  LatticeView L;         // (the whole lattice: gx0 == 0, nxl == lx)
  Kin K;
  double nu8, nu9;
  double* out;           // the planes
  long off[FL_FIELDS];   // where each field's plane starts in `out`; -1: not selected
  double* part;          // [lx][nb][8] per (row, block); null: no sums
  int nb;                // blocks of 64 y per row
};

// what a node yields when it is read
struct FlowVel { double ux, uy, rho, jx, jy, pxx, pxy; int fluid; };

__device__ __forceinline__ FlowVel flow_vel(const FlowJob& J, int x, int y) {
  const LatticeView& L = J.L;
  real f[9];
  const NodeVel N = node_vel(J.f, J.obst[(long)x * L.sy + y], L, J.K, x, y, f);   // (lbm_device.h: shared with the tracers)
  FlowVel V{N.ux, N.uy, N.rho, N.jx, N.jy, 0., 0., N.fluid};
  if (N.fluid) {
    const NodeMoments P = node_moments(f);   // (lbm_device.h: shared with the time averages)
    V.pxx = P.pxx;
    V.pxy = P.pxy;
  }
  return V;
}

// a lattice row as the march keeps it: the velocity of the lane's node and of its two neighbours in y, and what the sums need
struct FlowRow { double ux, uy, uxm, uxp, uym, uyp, rho, ke, diss, gdot, u2; int fluid; };

__global__ __launch_bounds__(FL_THREADS) void k_flow_nodes(const FlowJob J) {
  __shared__ double sS[FL_WAVES][FL_CHAINS][FL_PITCH];
  const LatticeView& L = J.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.x * FL_THREADS + threadIdx.x;
  const int xa = blockIdx.y * FL_SEG;
  const int xb = xa + FL_SEG < L.lx ? xa + FL_SEG : L.lx;
  const bool in = y < L.ly;
  const int yh = lane == 0 ? y - 1 : y + 1;   // the halo column of a wave's first and last lane
  const bool halo = (lane == 0 || lane == 63) && yh >= 0 && yh < L.ly;
  const long cnt_row = L.ly;
  FlowRow prev{}, cur{};
  for (int xr = xa - 1; xr <= xb; ++xr) {   // (every lane stays in the loop: wave shifts, barriers)
    FlowRow nx{};
    if (xr >= 0 && xr < L.lx) {
      FlowVel V{0., 0., 0., 0., 0., 0., 0., 0};
      if (in) V = flow_vel(J, xr, y);
      double hux = 0., huy = 0.;
      if (halo) {
        const FlowVel H = flow_vel(J, xr, yh);
        hux = H.ux; huy = H.uy;
      }
      nx.ux = V.ux; nx.uy = V.uy;
      nx.uxm = __shfl_up(V.ux, 1); nx.uym = __shfl_up(V.uy, 1);
      nx.uxp = __shfl_down(V.ux, 1); nx.uyp = __shfl_down(V.uy, 1);
      if (lane == 0) { nx.uxm = hux; nx.uym = huy; }
      if (lane == 63) { nx.uxp = hux; nx.uyp = huy; }
      if (xr >= xa && xr < xb) {   // a row of the segment: its local fields
        double nxx = 0., nxy = 0.;
        if (V.fluid) {
          const NodeStress S = node_stress(L, J.nu8, J.nu9, V.pxx, V.pxy, V.rho, V.jx, V.jy);   // (lbm_device.h, likewise)
          nxx = S.nxx;
          nxy = S.nxy;
          nx.gdot = S.gdot;
          nx.diss = S.diss;
          nx.u2 = V.ux * V.ux + V.uy * V.uy;
          nx.ke = 0.5 * V.rho * nx.u2;
          nx.rho = V.rho;
          nx.fluid = 1;
        }
        if (in) {
          const long at = (long)xr * cnt_row + y;
          if (J.off[0] >= 0) J.out[J.off[0] + at] = V.ux;
          if (J.off[1] >= 0) J.out[J.off[1] + at] = V.uy;
          if (J.off[4] >= 0) J.out[J.off[4] + at] = nxx;
          if (J.off[5] >= 0) J.out[J.off[5] + at] = nxy;
          if (J.off[6] >= 0) J.out[J.off[6] + at] = nx.gdot;
          if (J.off[7] >= 0) J.out[J.off[7] + at] = nx.diss;
        }
      }
    }
    const int xc = xr - 1;   // `cur` is row xc: with `prev` and `nx` around it, it is complete
    if (xc >= xa) {          // (xc < xb: xr <= xb)
      double vort = 0., div = 0.;
      if (in && xc >= 1 && xc <= L.lx - 2 && y >= 1 && y <= L.ly - 2) {
        vort = (nx.uy - prev.uy) * 0.5 - (cur.uxp - cur.uxm) * 0.5;
        div = (nx.ux - prev.ux) * 0.5 + (cur.uyp - cur.uym) * 0.5;
      }
      if (in) {
        const long at = (long)xc * cnt_row + y;
        if (J.off[2] >= 0) J.out[J.off[2] + at] = vort;
        if (J.off[3] >= 0) J.out[J.off[3] + at] = div;
      }
      if (J.part) {   // the chains of (row xc, this wave's block): a node that is not fluid holds +0.0
        const bool fl = cur.fluid != 0;   // (false beyond the lattice)
        sS[wave][0][lane] = fl ? cur.rho : 0.;
        sS[wave][1][lane] = fl ? cur.ke : 0.;
        sS[wave][2][lane] = fl ? cur.diss : 0.;
        sS[wave][3][lane] = fl ? 0.5 * vort * vort : 0.;
        sS[wave][4][lane] = fl ? cur.u2 : 0.;
        sS[wave][5][lane] = fl ? cur.gdot : 0.;
        sS[wave][6][lane] = fl ? fabs(div) : 0.;
        const unsigned long long fluid_lanes = __ballot(fl);
        __syncthreads();
        const int yw = y - lane;   // the block's first column
        if (yw < L.ly && lane < FL_SUMS) {
          double a = 0.;
          const double* s = sS[wave][lane < FL_CHAINS ? lane : 0];
          for (int k = 0; k < FL_BLOCK; ++k) {   // (one loop for the adding and the maximising lanes: the chain's latency once)
            const double v = s[k];
            a = lane < 4 ? a + v : fmax(a, v);
          }
          if (lane == FL_CHAINS) a = (double)__popcll(fluid_lanes);
          // record: n_fluid, then the seven chains
          J.part[((long)xc * J.nb + yw / FL_BLOCK) * FL_SUMS + (lane == FL_CHAINS ? 0 : lane + 1)] = a;
        }
        __syncthreads();   // the addends are overwritten in the next round
      }
    }
    prev = cur;
    cur = nx;
  }
}

// rows[x][k]: the chain of row x's block values, blocks ascending (k = 0: the count; 1..4: sums; 5..7: maxima)
__global__ __launch_bounds__(256) void k_flow_rows(const double* __restrict__ part, int lx, int nb, double* __restrict__ rows) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)lx * FL_SUMS) return;
  const int k = (int)(id % FL_SUMS);
  const double* p = part + (id / FL_SUMS) * nb * FL_SUMS + k;
  double a = 0.;
  if (k < 5) { for (int b = 0; b < nb; ++b) a += p[(long)b * FL_SUMS]; }
  else { for (int b = 0; b < nb; ++b) a = fmax(a, p[(long)b * FL_SUMS]); }
  rows[id] = a;
}

// sums[k]: the chain of the row values over x ascending. One workgroup: 256 rows at a time through LDS, eight lanes add serially.
__global__ __launch_bounds__(256) void k_flow_total(const double* __restrict__ rows, int lx, double* __restrict__ sums) {
  __shared__ double sR[256 * FL_SUMS];
  const int t = threadIdx.x;
  double a = 0.;
  for (int x0 = 0; x0 < lx; x0 += 256) {
    const int nr = lx - x0 < 256 ? lx - x0 : 256;
    for (int e = t; e < nr * FL_SUMS; e += 256) sR[e] = rows[(long)x0 * FL_SUMS + e];
    __syncthreads();
    if (t < FL_SUMS) {
      if (t < 5) { for (int r = 0; r < nr; ++r) a += sR[r * FL_SUMS + t]; }
      else { for (int r = 0; r < nr; ++r) a = fmax(a, sR[r * FL_SUMS + t]); }
    }
    __syncthreads();
  }
  if (t < FL_SUMS) sums[t] = a;
}

// The file's payloads from five planes (ux, uy, vort, gdot, diss; [lx][ly], `plane` doubles apart): the vector [ly][lx][3], then
// three scalars [ly][lx], big-endian float. A workgroup owns a tile of 32 x 32 nodes: in, lanes along y; out, lanes along x.
constexpr int IM_T = 32, IM_PITCH = IM_T + 1;
__global__ __launch_bounds__(256) void k_flow_image(const double* __restrict__ planes, long plane, int lx, int ly,
                                                    unsigned* __restrict__ image) {
  __shared__ float sT[5][IM_T][IM_PITCH];   // [plane][y][x]
  const int x0 = blockIdx.x * IM_T, y0 = blockIdx.y * IM_T;
#pragma unroll
  for (int it = 0; it < IM_T * IM_T / 256; ++it) {
    const int idx = it * 256 + threadIdx.x;
    const int yl = idx % IM_T, xl = idx / IM_T;
    if (x0 + xl < lx && y0 + yl < ly) {
      const long at = (long)(x0 + xl) * ly + (y0 + yl);
#pragma unroll
      for (int p = 0; p < 5; ++p) sT[p][yl][xl] = (float)planes[p * plane + at];
    }
  }
  __syncthreads();
  const size_t cnt = (size_t)lx * ly;
#pragma unroll
  for (int it = 0; it < IM_T * IM_T * 3 / 256; ++it) {
    const int e = it * 256 + threadIdx.x;
    const int yl = e / (IM_T * 3), j = e % (IM_T * 3), xl = j / 3, comp = j % 3;
    if (x0 + xl < lx && y0 + yl < ly) {
      const float v = comp < 2 ? sT[comp][yl][xl] : 0.f;
      image[((size_t)(y0 + yl) * lx + x0) * 3 + j] = __builtin_bswap32(__float_as_uint(v));
    }
  }
#pragma unroll
  for (int p = 2; p < 5; ++p)
#pragma unroll
    for (int it = 0; it < IM_T * IM_T / 256; ++it) {
      const int e = it * 256 + threadIdx.x;
      const int yl = e / IM_T, xl = e % IM_T;
      if (x0 + xl < lx && y0 + yl < ly)
        image[(size_t)(p + 1) * cnt + (size_t)(y0 + yl) * lx + x0 + xl] = __builtin_bswap32(__float_as_uint(sT[p][yl][xl]));
    }
}

int popcount8(int mask) {
  int c = 0;
  for (int b = 0; b < FL_FIELDS; ++b) c += (mask >> b) & 1;
  return c;
}

// the node kernel on the handle's stream: the planes of `mask` to dev_out (device memory), the partial sums when `sums`
int flow_launch(lbmdem_handle* h, int mask, double* dev_out, bool sums) {
  const LatticeView& L = h->L;
  const long cnt = (long)L.lx * L.ly;
  FlowJob J{};
  J.f = h->f[h->fcur];
  J.obst = reader_obst(h);
  J.L = L;
  J.L.gate = nullptr;
  J.K = h->kin[h->kcur];
  const double s8 = h->cfg.phys.s8, s9 = h->cfg.phys.s9;
  J.nu8 = (1. / s8 - 0.5) / 3.;
  J.nu9 = (1. / s9 - 0.5) / 3.;
  J.out = dev_out;
  int nsel = 0;
  for (int b = 0; b < FL_FIELDS; ++b) J.off[b] = ((mask >> b) & 1) ? (long)(nsel++) * cnt : -1;
  J.nb = (L.ly + FL_BLOCK - 1) / FL_BLOCK;
  J.part = nullptr;
  if (sums) {
    auto& S = h->fl;
    HIP_TRY(h->mem.grow(&S.part, &S.part_cap, (long)L.lx * J.nb * FL_SUMS + (long)L.lx * FL_SUMS));
    if (!S.sums) HIP_TRY(h->mem.dev(&S.sums, (size_t)FL_SUMS));
    J.part = S.part;
  }
  hipLaunchKernelGGL(k_flow_nodes, dim3((L.ly + FL_THREADS - 1) / FL_THREADS, (L.lx + FL_SEG - 1) / FL_SEG), dim3(FL_THREADS), 0,
                     h->stream, J);
  HIP_TRY(hipGetLastError());
  if (sums) {
    auto& S = h->fl;
    double* rows = S.part + (long)L.lx * J.nb * FL_SUMS;
    hipLaunchKernelGGL(k_flow_rows, dim3((unsigned)(((long)L.lx * FL_SUMS + 255) / 256)), dim3(256), 0, h->stream, S.part, L.lx,
                       J.nb, rows);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_flow_total, dim3(1), dim3(256), 0, h->stream, rows, L.lx, S.sums);
    HIP_TRY(hipGetLastError());
  }
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

// flow%.6i.vtk from the payloads in file byte order: [ly][lx][3] words of the vector, then three scalars [ly][lx]
int flow_write_image(const char* dir, int nfile, int lx, int ly, const unsigned* image) {
  static const char* const NAMES[3] = {"vorticity", "shear_rate", "dissipation"};
  OutFile F;
  RC_TRY(F.open("w+", dir, "flow%.6i.vtk", nfile));
  FILE* fp = F.fp;
  const size_t cnt = (size_t)lx * ly;
  lbmdem_vtk_put_mesh(fp, lx, ly);
  fprintf(fp, "VECTORS fluid_velocity_lb float\n");
  bool short_write = fwrite(image, 4, 3 * cnt, fp) != 3 * cnt;
  for (int k = 0; k < 3 && !short_write; ++k) {
    fprintf(fp, "SCALARS %s float\nLOOKUP_TABLE default\n", NAMES[k]);
    short_write = fwrite(image + (3 + k) * cnt, 4, cnt, fp) != cnt;
  }
  return F.close(short_write);
}

inline unsigned be_float(double v) {
  const float f = (float)v;
  unsigned u;
  memcpy(&u, &f, 4);
  return __builtin_bswap32(u);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_flow_files(const char* dir, int nfile, int lx, int ly, const double* ux, const double* uy, const double* vort,
                            const double* gdot, const double* diss) try {
  if (!ux || !uy || !vort || !gdot || !diss) return fail(LBMDEM_EINVAL, "null buffer");
  if (lx < 2 || ly < 2) return fail(LBMDEM_EINVAL, "lbmdem_write_flow_files: the lattice is %d x %d", lx, ly);
  const size_t cnt = (size_t)lx * ly;
  std::vector<unsigned> image(FL_FILE_WORDS * cnt);
  const double* scal[3] = {vort, gdot, diss};
  for (int y = 0; y < ly; ++y)
    for (int x = 0; x < lx; ++x) {
      const size_t in = (size_t)x * ly + y, o = (size_t)y * lx + x;
      image[3 * o] = be_float(ux[in]);
      image[3 * o + 1] = be_float(uy[in]);
      image[3 * o + 2] = be_float(0.);
      for (int k = 0; k < 3; ++k) image[(3 + k) * cnt + o] = be_float(scal[k][in]);
    }
  return flow_write_image(dir, nfile, lx, ly, image.data());
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_flow_fields(lbmdem_handle* h, int, double*, long, long*) { SP_REFUSE(h, "the flow fields export"); }
int lbmdem_flow_fields_device(lbmdem_handle* h, int, void*, long) { SP_REFUSE(h, "the flow fields export"); }
int lbmdem_flow_sums(lbmdem_handle* h, double*) { SP_REFUSE(h, "the flow fields export"); }
int lbmdem_write_flow(lbmdem_handle* h, const char*, int) { SP_REFUSE(h, "the flow fields export"); }
int lbmdem_set_flow_output(lbmdem_handle* h, int) { SP_REFUSE(h, "the flow fields export"); }
#else

int lbmdem_flow_fields_device(lbmdem_handle* h, int mask, void* dev_out, long cap_doubles) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_flow_fields_device"));
  if (mask <= 0 || (mask & ~LBMDEM_FLOW_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_flow_fields_device: bad mask %d", mask);
  if (!dev_out) return fail(LBMDEM_EINVAL, "null buffer");
  const long need = (long)popcount8(mask) * h->L.lx * h->L.ly;
  if (cap_doubles < need)
    return fail(LBMDEM_EINVAL, "lbmdem_flow_fields_device: the planes are %ld doubles, the buffer holds %ld", need, cap_doubles);
  return flow_launch(h, mask, static_cast<double*>(dev_out), false);
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_flow_fields(lbmdem_handle* h, int mask, double* out, long cap_doubles, long* count) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_flow_fields"));
  if (mask <= 0 || (mask & ~LBMDEM_FLOW_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_flow_fields: bad mask %d", mask);
  if (!count || cap_doubles < 0 || (cap_doubles > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  const long need = (long)popcount8(mask) * h->L.lx * h->L.ly;
  *count = need;
  if (cap_doubles == 0) return LBMDEM_OK;   // (how many there are)
  if (cap_doubles < need)
    return fail(LBMDEM_EINVAL, "lbmdem_flow_fields: the planes are %ld doubles, the buffer holds %ld", need, cap_doubles);
  auto& S = h->fl;
  HIP_TRY(h->mem.grow(&S.planes, &S.planes_cap, need));
  RC_TRY(flow_launch(h, mask, S.planes, false));
  HIP_TRY(hipMemcpyAsync(out, S.planes, sizeof(double) * (size_t)need, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_flow_sums(lbmdem_handle* h, double* sums8) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_flow_sums"));
  if (!sums8) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(flow_launch(h, 0, nullptr, true));
  HIP_TRY(hipMemcpyAsync(sums8, h->fl.sums, sizeof(double) * FL_SUMS, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_flow(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_write_flow"));
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  const LatticeView& L = h->L;
  const long cnt = (long)L.lx * L.ly;
  auto& S = h->fl;
  HIP_TRY(h->mem.grow(&S.planes, &S.planes_cap, 5 * cnt));
  HIP_TRY(h->mem.grow(&S.image, &S.image_cap, FL_FILE_WORDS * cnt));
  RC_TRY(flow_launch(h, LBMDEM_FLOW_UX | LBMDEM_FLOW_UY | LBMDEM_FLOW_VORT | LBMDEM_FLOW_GDOT | LBMDEM_FLOW_DISS, S.planes, false));
  hipLaunchKernelGGL(k_flow_image, dim3((L.lx + IM_T - 1) / IM_T, (L.ly + IM_T - 1) / IM_T), dim3(256), 0, h->stream, S.planes, cnt,
                     L.lx, L.ly, S.image);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned> image((size_t)FL_FILE_WORDS * cnt);
  HIP_TRY(hipMemcpyAsync(image.data(), S.image, sizeof(unsigned) * image.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return flow_write_image(dir, nfile, L.lx, L.ly, image.data());
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_flow_output(lbmdem_handle* h, int on) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) RC_TRY(whole_handle(h, "lbmdem_set_flow_output"));
  h->flow_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
