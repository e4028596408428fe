// lbm_coarse.hip -- coarse-grained fields (lbmdem_coarse_grid, lbmdem_coarse_fields, lbmdem_write_coarse, lbmdem_write_coarse_files,
// lbmdem_set_coarse_output; include/lbmdem_hip.h): per cell of cw x ch lattice nodes the sums people plot -- node counts by class,
// rho, j and pore pressure over the fluid nodes; mass, momentum, kinetic energy and hydrodynamic force of the grains whose centre
// lies in the cell; coordination, pressure and moment tensor of the last table sub-step. The reference has no such routine (its
// write_DEM adds some of these over the whole packing, main.c:373-421), so the contract is exact arithmetic: every number is a chain
// of additions in a fixed order, which a serial loop reproduces bit for bit. Nothing here is on the step path: the kernels only
// read the handle's state.
//
// Node block, two kernels, no atomics:
//   k_coarse_rows   a workgroup owns one lattice row x and walks it in chunks of 256 y, lanes along y (the contiguous axis of
//                   f[x][y / 16][q][y % 16] and obst[x][y]): rho, jx, jy, P and the node's class go to LDS, then ONE lane per
//                   cell segment [cy * ch, (cy + 1) * ch) of the chunk adds its values serially, y ascending. A segment that
//                   spans chunks stays with its lane (cy mod 256), which carries the sums in registers: one column sum per (x, cy);
//   k_coarse_cells  one lane per cell chains the at most cw column sums over x ascending.
// Grain block: k_coarse_keys gives every grain the index of its cell (or the sentinel `ncells`: outside), a stable radix sort of
// (key, grain index) keeps a cell's grains in index order, and in k_coarse_grains one lane per cell finds its segment of the sorted
// keys by bisection and walks it serially. A cell without grains writes zeros.
// Double-precision library only: the entry points that take a handle refuse in the float build. Grid arithmetic and the file's
// formatter are host code and exist in both.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h) for the refusals and the map,
// MemPool::grow (lbm_mem.h) for the scratch kept on the handle, OutFile (lbm_outfile.h) for the file.
#include "lbm_device.h"
#include "lbm_outfile.h"

#include <errno.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

static_assert(sizeof(lbmdem_coarse_cell) == LBMDEM_COARSE_DOUBLES * sizeof(double), "lbmdem_coarse_cell is 25 doubles, no padding");
constexpr int CG_REC = LBMDEM_COARSE_DOUBLES;

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int CG_THREADS = 256;                  // nodes of a chunk; also the most cell segments a chunk can hold (ch == 1)
// LDS: a node's value at y + y / 16 -- one double of padding per 16 -- so that the lanes of a chunk's segments, ch doubles apart,
// do not all start on one bank when ch is a multiple of 16 (ch == 16: 17 doubles = 34 words apart, 16 lanes on 16 bank pairs)
__device__ __forceinline__ int cg_pad(int k) { return k + (k >> 4); }
constexpr int CG_PITCH = CG_THREADS + CG_THREADS / 16;
constexpr int CG_COL = 7;                        // per (x, cy): fluid, grain, wall nodes, then the sums of rho, jx, jy, P

struct CoarseJob {
  // nodes
  const real* f;
  const int* obst;       // the map the last fluid step saw, device layout [x][sy]
  LatticeView L;         // (the whole lattice: gx0 == 0, nxl == lx)
  real rho_moy;
  int cw, ch, ncx, ncy;
  double* col;           // [lx][CG_COL][ncy] column sums
  double* out;           // [ncx * ncy][CG_REC] the records
  // grains
  int n;
  Kin K;
  const real *m, *It, *fhf;
  real Mgx, Mby, dx;
  unsigned *keys;        // k_coarse_keys: [n]; k_coarse_grains: the sorted ones
  int* idx;              // ... and the grain indices that go with them
  unsigned ncells;       // the key of a grain outside
  int table;             // the last sub-step was a table sub-step: the contact block is read
  const int* z;
  const real *p, *M;     // M: [4][n] M11 M12 M21 M22
  long long* outside;    // [1]
};

__global__ __launch_bounds__(CG_THREADS) void k_coarse_rows(const CoarseJob J) {
  __shared__ double sV[4][CG_PITCH];
  __shared__ int sC[CG_THREADS];   // 0 fluid, 1 grain, 2 wall, 3 none of them or beyond the lattice
  const LatticeView& L = J.L;
  const int x = blockIdx.x, t = threadIdx.x;
  double a_rho = 0., a_jx = 0., a_jy = 0., a_P = 0.;
  int n_fluid = 0, n_grain = 0, n_wall = 0;
  for (int y0 = 0; y0 < L.ly; y0 += CG_THREADS) {   // (every lane stays in the loop: barriers)
    const int y = y0 + t;
    real rho = 0., jx = 0., jy = 0., P = 0.;
    int cls = 3;
    if (y < L.ly) {
      const long node = (long)x * L.sy + y;
      const int o = J.obst[node];
      if (o == -1) {
        cls = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          const real v = J.f[fidx(i, node)];
          rho += v;
          jx += v * EXq(i);
          jy += v * EYq(i);
        }
        P = (1. / 3.) * J.rho_moy * (rho - 1.);   // main.c:320, 533
      } else if (o >= 0 && o < L.n) {
        cls = 1;
      } else if (o == L.n) {
        cls = 2;
      }
    }
    const int pt = cg_pad(t);
    sV[0][pt] = rho; sV[1][pt] = jx; sV[2][pt] = jy; sV[3][pt] = P;
    sC[t] = cls;
    __syncthreads();
    // the segments that meet this chunk are c0 .. c1, at most CG_THREADS of them: lane t has the one with c % CG_THREADS == t
    const int y1 = y0 + CG_THREADS < L.ly ? y0 + CG_THREADS : L.ly;
    const int c0 = y0 / J.ch, c1 = (y1 - 1) / J.ch;
    const int c = c0 + (t - c0 % CG_THREADS + CG_THREADS) % CG_THREADS;
    if (c <= c1) {
      const int s0 = c * J.ch;   // (<= y1 - 1)
      const int s1 = J.ch < L.ly - s0 ? s0 + J.ch : L.ly;
      if (s0 >= y0) {   // it begins here; otherwise this lane has carried it from the chunk before
        a_rho = 0.; a_jx = 0.; a_jy = 0.; a_P = 0.;
        n_fluid = 0; n_grain = 0; n_wall = 0;
      }
      const int b = (s0 > y0 ? s0 : y0) - y0, e = (s1 < y1 ? s1 : y1) - y0;
      for (int k = b; k < e; ++k) {   // a node that is not fluid holds +0.0
        const int pk = cg_pad(k);
        a_rho += sV[0][pk]; a_jx += sV[1][pk]; a_jy += sV[2][pk]; a_P += sV[3][pk];
        const int cl = sC[k];
        n_fluid += cl == 0; n_grain += cl == 1; n_wall += cl == 2;
      }
      if (s1 <= y1) {   // ... and ends here
        double* o = J.col + (long)x * CG_COL * J.ncy + c;
        o[0] = n_fluid; o[J.ncy] = n_grain; o[2L * J.ncy] = n_wall;
        o[3L * J.ncy] = a_rho; o[4L * J.ncy] = a_jx; o[5L * J.ncy] = a_jy; o[6L * J.ncy] = a_P;
      }
    }
    __syncthreads();   // the chunk's values are overwritten in the next round
  }
}

__global__ __launch_bounds__(CG_THREADS) void k_coarse_cells(const CoarseJob J) {
  const long cell = (long)blockIdx.x * CG_THREADS + threadIdx.x;   // lanes along cy: the column sums of one x are consecutive
  if (cell >= (long)J.ncx * J.ncy) return;
  const int cy = (int)(cell % J.ncy), cx = (int)(cell / J.ncy);
  const int x0 = cx * J.cw;
  const int x1 = J.cw < J.L.lx - x0 ? x0 + J.cw : J.L.lx;
  double a[CG_COL];
#pragma unroll
  for (int q = 0; q < CG_COL; ++q) a[q] = 0.;
  for (int x = x0; x < x1; ++x) {
    const double* c = J.col + (long)x * CG_COL * J.ncy + cy;
#pragma unroll
    for (int q = 0; q < CG_COL; ++q) a[q] += c[(long)q * J.ncy];
  }
  double* o = J.out + cell * CG_REC;
  o[0] = a[0] + a[1] + a[2];   // (counts: small integers, exact in any order)
  o[1] = a[0]; o[2] = a[1]; o[3] = a[2];
  o[4] = a[3]; o[5] = a[4]; o[6] = a[5]; o[7] = a[6];
}

// the cell of a grain's centre in node coordinates as the rasteriser forms them (main.c:1009-1010)
__global__ __launch_bounds__(CG_THREADS) void k_coarse_keys(const CoarseJob J) {
  const int i = blockIdx.x * CG_THREADS + threadIdx.x;
  if (i >= J.n) return;
  const real xc = (J.K.x1[i] - J.Mgx) / J.dx, yc = (J.K.x2[i] - J.Mby) / J.dx;
  unsigned key = J.ncells;
  if (xc >= 0 && xc < J.L.lx && yc >= 0 && yc < J.L.ly)   // (false for NaN)
    key = (unsigned)((int)xc / J.cw) * (unsigned)J.ncy + (unsigned)((int)yc / J.ch);
  J.keys[i] = key;
  J.idx[i] = i;
}

// the first position of the sorted keys that holds `key` or more
__device__ __forceinline__ int cg_lower_bound(const unsigned* keys, int n, unsigned key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(CG_THREADS) void k_coarse_grains(const CoarseJob J) {
  const long cell = (long)blockIdx.x * CG_THREADS + threadIdx.x;
  if (cell >= (long)J.ncells) return;
  const int p0 = cg_lower_bound(J.keys, J.n, (unsigned)cell), p1 = cg_lower_bound(J.keys, J.n, (unsigned)cell + 1u);
  if (cell + 1 == (long)J.ncells) *J.outside = J.n - p1;   // (behind the last cell: the sentinel's grains)
  double cnt = 0., s_m = 0., s_mv1 = 0., s_mv2 = 0., s_Iw = 0., kx = 0., ky = 0., kt = 0., h1 = 0., h2 = 0., h3 = 0.;
  double s_z = 0., s_p = 0., M11 = 0., M12 = 0., M21 = 0., M22 = 0.;
  const size_t n = (size_t)J.n;
  for (int p = p0; p < p1; ++p) {   // ascending grain index: the sort is stable
    const int i = J.idx[p];
    const real m = J.m[i], It = J.It[i], v1 = J.K.v1[i], v2 = J.K.v2[i], v3 = J.K.v3[i];
    cnt += 1.;
    s_m += m; s_mv1 += m * v1; s_mv2 += m * v2; s_Iw += It * v3;
    kx += 0.5 * m * v1 * v1; ky += 0.5 * m * v2 * v2; kt += 0.5 * It * v3 * v3;   // main.c:381-383
    h1 += J.fhf[i]; h2 += J.fhf[n + i]; h3 += J.fhf[2 * n + i];
    if (J.table) {
      s_z += (double)J.z[i]; s_p += J.p[i];
      M11 += J.M[i]; M12 += J.M[n + i]; M21 += J.M[2 * n + i]; M22 += J.M[3 * n + i];
    }
  }
  double* o = J.out + cell * CG_REC + 8;
  o[0] = cnt; o[1] = s_m; o[2] = s_mv1; o[3] = s_mv2; o[4] = s_Iw; o[5] = kx; o[6] = ky; o[7] = kt;
  o[8] = h1; o[9] = h2; o[10] = h3;
  o[11] = s_z; o[12] = s_p; o[13] = M11; o[14] = M12; o[15] = M21; o[16] = M22;
}

int sort_bits(unsigned ncells) {   // the keys are 0 .. ncells
  int b = 1;
  while (b < 32 && (ncells >> b) != 0) ++b;
  return b;
}

// scratch of the handle's pool, made by the first call, grown when a finer grid asks for more, freed with the handle
int coarse_stage(lbmdem_handle* h, long ncells, long ncol, int bits) {
  auto& S = h->cg;
  const int n = h->n;
  HIP_TRY(h->mem.grow(&S.cells, &S.cell_cap, ncells * CG_REC));
  HIP_TRY(h->mem.grow(&S.col, &S.col_cap, ncol));
  if (!S.keys[0]) {
    HIP_TRY(h->mem.dev(&S.keys[0], (size_t)n));
    HIP_TRY(h->mem.dev(&S.keys[1], (size_t)n));
    HIP_TRY(h->mem.dev(&S.idx[0], (size_t)n));
    HIP_TRY(h->mem.dev(&S.idx[1], (size_t)n));
    HIP_TRY(h->mem.dev(&S.outside, 1));
  }
  size_t bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, S.keys[0], S.keys[1], S.idx[0], S.idx[1], n, 0, bits, h->stream));
  HIP_TRY(h->mem.grow(&S.sort_tmp, &S.sort_bytes, (long)bytes));
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

int grid_of(int lx, int ly, int cw, int ch, int* ncx, int* ncy) {
  if (lx < 1 || ly < 1) return fail(LBMDEM_EINVAL, "lbmdem_coarse_grid: the lattice is %d x %d", lx, ly);
  if (cw < 1 || ch < 1) return fail(LBMDEM_EINVAL, "a coarse cell must hold at least one node each way (cw = %d, ch = %d)", cw, ch);
  *ncx = (int)(((long)lx + cw - 1) / cw);
  *ncy = (int)(((long)ly + ch - 1) / ch);
  return LBMDEM_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_coarse_grid(int lx, int ly, int cw, int ch, int* ncx, int* ncy) {
  if (!ncx || !ncy) return fail(LBMDEM_EINVAL, "null argument");
  return grid_of(lx, ly, cw, ch, ncx, ncy);
}

int lbmdem_write_coarse_files(const char* dir, int nfile, int lx, int ly, int cw, int ch, const lbmdem_coarse_cell* cells,
                              long outside, int contacts_valid) {
  if (!cells) return fail(LBMDEM_EINVAL, "null buffer");
  int ncx = 0, ncy = 0;
  RC_TRY(grid_of(lx, ly, cw, ch, &ncx, &ncy));
  OutFile F;
  RC_TRY(F.open("w", dir, "coarse%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# cw %d ch %d ncx %d ncy %d outside %ld contacts %d\n", cw, ch, ncx, ncy, outside, contacts_valid);
  for (int cx = 0; cx < ncx; ++cx)
    for (int cy = 0; cy < ncy; ++cy) {
      const double* v = reinterpret_cast<const double*>(cells + (size_t)cx * ncy + cy);
      fprintf(fp, "%d %d", cx, cy);
      for (int k = 0; k < CG_REC; ++k) fprintf(fp, " %le", v[k]);
      fprintf(fp, "\n");
    }
  return F.close();
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_coarse_fields(lbmdem_handle* h, int, int, lbmdem_coarse_cell*, long, long*, long*) { SP_REFUSE(h, "the coarse-grained fields export"); }
int lbmdem_write_coarse(lbmdem_handle* h, const char*, int, int, int) { SP_REFUSE(h, "the coarse-grained fields export"); }
int lbmdem_set_coarse_output(lbmdem_handle* h, int, int) { SP_REFUSE(h, "the coarse-grained fields export"); }
#else

int lbmdem_coarse_fields(lbmdem_handle* h, int cw, int ch, lbmdem_coarse_cell* out, long cap_cells, long* count, long* info2) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!count || !info2 || cap_cells < 0 || (cap_cells > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_coarse_fields"));
  const LatticeView& L = h->L;
  int ncx = 0, ncy = 0;
  RC_TRY(grid_of(L.lx, L.ly, cw, ch, &ncx, &ncy));
  const long ncells = (long)ncx * ncy;
  *count = ncells;
  if (cap_cells == 0) return LBMDEM_OK;   // (how many there are)
  if (cap_cells < ncells) return fail(LBMDEM_EINVAL, "lbmdem_coarse_fields: there are %ld cells, the buffer holds %ld", ncells, cap_cells);
  const int n = h->n, bits = sort_bits((unsigned)ncells);
  RC_TRY(coarse_stage(h, ncells, (long)L.lx * CG_COL * ncy, bits));
  auto& S = h->cg;
  CoarseJob J{};
  J.f = h->f[h->fcur];
  J.obst = reader_obst(h);
  J.L = L;
  J.L.gate = nullptr;
  J.rho_moy = (real)h->cfg.phys.rho_moy;
  J.cw = cw; J.ch = ch; J.ncx = ncx; J.ncy = ncy;
  J.col = S.col;
  J.out = S.cells;
  J.n = n;
  J.K = h->kin[h->kcur];
  J.m = h->m; J.It = h->It; J.fhf = h->fhf;
  J.Mgx = (real)h->cfg.Mgx; J.Mby = (real)h->cfg.Mby; J.dx = (real)h->cfg.dx;   // the walls lbmdem_get_walls reports
  J.keys = S.keys[0]; J.idx = S.idx[0];
  J.ncells = (unsigned)ncells;
  J.table = h->diag_valid ? 1 : 0;   // lbmdem_download_grain_table's own condition
  if (J.table) {   // h->diag: [8][n] reals, M11 .. M22 the last four, then z as ints
    J.z = reinterpret_cast<const int*>(h->diag + 8 * (size_t)n);
    J.p = h->gp;
    J.M = h->diag + 4 * (size_t)n;
  }
  J.outside = S.outside;
  const int cell_blocks = (int)((ncells + CG_THREADS - 1) / CG_THREADS);
  hipLaunchKernelGGL(k_coarse_rows, dim3(L.lx), dim3(CG_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_coarse_cells, dim3(cell_blocks), dim3(CG_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_coarse_keys, dim3((n + CG_THREADS - 1) / CG_THREADS), dim3(CG_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  size_t bytes = (size_t)S.sort_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(S.sort_tmp, bytes, S.keys[0], S.keys[1], S.idx[0], S.idx[1], n, 0, bits, h->stream));
  J.keys = S.keys[1]; J.idx = S.idx[1];
  hipLaunchKernelGGL(k_coarse_grains, dim3(cell_blocks), dim3(CG_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  long long outside = 0;
  HIP_TRY(hipMemcpyAsync(out, S.cells, sizeof(lbmdem_coarse_cell) * (size_t)ncells, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&outside, S.outside, sizeof outside, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  info2[0] = (long)outside;
  info2[1] = J.table;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_coarse(lbmdem_handle* h, const char* dir, int nfile, int cw, int ch) try {
  CHECK_H(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  long count = 0, info[2] = {0, 0};
  RC_TRY(lbmdem_coarse_fields(h, cw, ch, nullptr, 0, &count, info));
  std::vector<lbmdem_coarse_cell> cells((size_t)count);
  RC_TRY(lbmdem_coarse_fields(h, cw, ch, cells.data(), count, &count, info));
  return lbmdem_write_coarse_files(dir, nfile, h->cfg.lx, h->cfg.ly, cw, ch, cells.data(), info[0], (int)info[1]);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_coarse_output(lbmdem_handle* h, int cw, int ch) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  const bool on = cw != 0 || ch != 0;
  if (on && (cw < 1 || ch < 1)) return fail(LBMDEM_EINVAL, "a coarse cell must hold at least one node each way (cw = %d, ch = %d)", cw, ch);
  if (on) RC_TRY(whole_handle(h, "lbmdem_set_coarse_output"));
  h->coarse_cw = cw;
  h->coarse_ch = ch;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
