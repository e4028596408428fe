// lbm_densities.hip -- write_densities (main.c:482-566; include/lbmdem_hip.h: lbmdem_write_densities,
// lbmdem_download_densities_text, lbmdem_set_densities_staging, lbmdem_densities_stats, lbmdem_write_densities_host,
// lbmdem_format_fixed4): the reference's ASCII dump of the fluid fields masked by the obstacle map -- densities%.6i.vtk, a
// Pressure section and a VecVelocity section of "%.4lf" text, file order [y][x] -- and pressure_base%.6i.dat, the profile of
// row y == 2. Nothing here is on the step path: the kernels only read f and the obstacle map.
//
// The text is made on the device (lbm_text.h: the exact four-decimal formatter). Lines have variable length, so, as for the
// boundary links (lbm_links.hip), the order of the file is fixed without atomics in three steps on the handle's stream:
//   k_dens_count   the length of every node's line in both sections, summed per cell -- one y, 64 consecutive x --; row 2's
//                  pressures; the number of nodes with a value the device does not format (non-finite or >= 1e9);
//   an exclusive scan over the cells of both sections in file order (hipcub::DeviceScan): byte offsets into the body;
//   k_dens_emit    the values once more, every cell's text staged in LDS and stored at its offset.
// The emit pass runs over BANDS of whole file rows of one section: a band's bytes are known from the scan, they go to a device
// staging buffer, from there to pinned host memory and on to the file, band after band in file order; both buffers are bounded
// by the staging budget (lbmdem_set_densities_staging), whatever the lattice. If a single node is refused the whole file is
// written by the host formatter (lbmdem_write_densities_host: the reference's loops, one fprintf per value) instead.
// Double-precision library only: the entry points that take a handle refuse in the float build.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h) for the refusals and the map,
// OutFile (lbm_outfile.h) for the two files -- closed together, with one text for the pair; the scratch is a call's own.
#include "lbm_device.h"
#include "lbm_outfile.h"
#include "lbm_text.h"

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

#ifndef LBMDEM_SINGLE_PRECISION
// A workgroup owns DN_BX lattice rows x one y-tile of the population layout (64 x 16 nodes, four per lane), as k_vtk_frame:
//   in:      lanes run along y first -- f[x][y / 16][q][y % 16] and obst[x][y] have y as the fast axis: a tile's nine directions
//            are nine consecutive 128-byte lines per x, every line used whole;
//   LDS:     P, u_x, u_y of every node as doubles, plane by plane, [y][x] with a padded pitch;
//   compute: lanes run along x first -- a wavefront holds one cell, the 64 consecutive x of one y, so that the order of the
//            file is the order of the lanes; the four wavefronts take every fourth y.
// LDS banking: the 8-byte stores of a group of 16 lanes go to 16 different y of one x, 2 * DN_PITCH * y words apart -- DN_PITCH
// odd gives the even banks 0, 2 .. 30 (mod 32), one pair per lane; the loads of a cell are consecutive.
constexpr int DN_TY = LBMDEM_TILE_Y, DN_BX = 64, DN_PITCH = DN_BX + 1, DN_PLANE = DN_TY * DN_PITCH;
// the longest line: two values of sign + 10 digits + '.' + 4 digits, two blanks, "0." and the newline
constexpr int DN_LINE = 2 * 16 + 5;
constexpr int DN_CELL = (DN_BX * DN_LINE + 3 + 15) / 16 * 16;   // a cell's text in LDS, begun at the alignment of its destination
static_assert(DN_BX == 64 && DN_TY == 16, "a cell is one wavefront, a workgroup four nodes per lane");

struct DensJob {
  const real* f;
  const int* obst;       // the map the last fluid step saw, device layout [x][sy]
  LatticeView L;         // (the whole lattice: gx0 == 0, nxl == lx)
  real rho_moy;
  int nxb;               // cells per file row
  long long ncell;       // cells per section: ly * nxb
  // count: [2 * ncell + 1] bytes per cell, the Pressure section's cells in file order, then the VecVelocity section's, then 0;
  // emit: their exclusive scan
  long long* cells;
  double* prow;          // count: [lx] P of row y == 2
  unsigned* refused;     // count: nodes with a value the device does not format
  // emit: file rows [y0, y1) of `section` (0 Pressure, 1 VecVelocity) to out[0 .. cap), which begins at byte `base` of the body
  int section, y0, y1;
  long long base, cap;
  unsigned char* out;
};

// P, u_x, u_y of the workgroup's nodes (main.c:524-528, 548-553) into the three planes; +0.0 where obst >= 0 (main.c:535,
// 559) and beyond the lattice
__device__ __forceinline__ void stage_values(const DensJob& J, double* sV, int x0, int y0) {
  const LatticeView& L = J.L;
#pragma unroll
  for (int it = 0; it < DN_BX * DN_TY / 256; ++it) {
    const int idx = it * 256 + threadIdx.x;
    const int yl = idx % DN_TY, xl = idx / DN_TY;
    const int x = x0 + xl, y = y0 + yl;
    real P = 0., u_x = 0., u_y = 0.;
    if (x < L.lx && y < L.ly) {
      const long node = (long)x * L.sy + y;
      if (J.obst[node] < 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          const real v = J.f[fidx(i, node)];
          P += v;
          u_x += v * EXq(i);
          u_y += v * EYq(i);
        }
        P = (1. / 3.) * J.rho_moy * (P - 1.);
      }
    }
    double* o = sV + yl * DN_PITCH + xl;
    o[0] = P; o[DN_PLANE] = u_x; o[2 * DN_PLANE] = u_y;
  }
}

__device__ __forceinline__ int wave_total(int v) { return __builtin_amdgcn_readlane(wave_inclusive_scan(v), 63); }

__global__ __launch_bounds__(256) void k_dens_count(const DensJob J) {
  __shared__ double sV[3 * DN_PLANE];
  const LatticeView& L = J.L;
  const int x0 = blockIdx.x * DN_BX, y0 = blockIdx.y * DN_TY;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  stage_values(J, sV, x0, y0);
  __syncthreads();
  for (int r = 0; r < DN_TY / 4; ++r) {   // (every lane of the wavefront stays in the loop: wave_total moves data between lanes)
    const int yl = wave + 4 * r, x = x0 + lane, y = y0 + yl;
    const bool in = x < L.lx && y < L.ly;
    const double P = sV[yl * DN_PITCH + lane], u_x = sV[DN_PLANE + yl * DN_PITCH + lane], u_y = sV[2 * DN_PLANE + yl * DN_PITCH + lane];
    const bool ok = fixed4_ok(P) && fixed4_ok(u_x) && fixed4_ok(u_y);
    int lp = 0, lv = 0;
    if (in && ok) {
      lp = fixed4_len(P) + 1;                        // "%.4lf\n"
      lv = fixed4_len(u_x) + fixed4_len(u_y) + 5;    // "%.4lf %.4lf 0.\n"
    }
    const int cp = wave_total(lp), cv = wave_total(lv), bad = wave_total(in && !ok ? 1 : 0);
    if (lane == 0 && y < L.ly) {
      J.cells[(long long)y * J.nxb + blockIdx.x] = cp;
      J.cells[J.ncell + (long long)y * J.nxb + blockIdx.x] = cv;
      if (bad) atomicAdd(J.refused, (unsigned)bad);
    }
    if (in && y == 2) J.prow[x] = P;
  }
}

__global__ __launch_bounds__(256) void k_dens_emit(const DensJob J) {
  __shared__ double sV[3 * DN_PLANE];
  __shared__ __attribute__((aligned(16))) unsigned char sT[4][DN_CELL];
  const LatticeView& L = J.L;
  const int x0 = blockIdx.x * DN_BX, y0 = (J.y0 / DN_TY + blockIdx.y) * DN_TY;   // (the tiles that hold rows of the band)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  stage_values(J, sV, x0, y0);
  __syncthreads();
  for (int r = 0; r < DN_TY / 4; ++r) {
    const int yl = wave + 4 * r, x = x0 + lane, y = y0 + yl;
    const bool row = y >= J.y0 && y < J.y1;   // (the same for every lane of the wavefront)
    const bool in = row && x < L.lx;
    const double P = sV[yl * DN_PITCH + lane], u_x = sV[DN_PLANE + yl * DN_PITCH + lane], u_y = sV[2 * DN_PLANE + yl * DN_PITCH + lane];
    const bool ok = fixed4_ok(P) && fixed4_ok(u_x) && fixed4_ok(u_y);   // (a refused node: the host writes the file, not this pass)
    int len = 0;
    if (in && ok) len = J.section == 0 ? fixed4_len(P) + 1 : fixed4_len(u_x) + fixed4_len(u_y) + 5;
    const int upto = wave_inclusive_scan(len);
    const int total = __builtin_amdgcn_readlane(upto, 63);
    // where the cell begins in the band; its text is staged at the same alignment, so that whole words of it are whole words there
    const long long at = row ? J.cells[J.section * J.ncell + (long long)y * J.nxb + blockIdx.x] - J.base : 0;
    const int al = (int)(at & 3);
    unsigned char* s = sT[wave] + al;
    if (len > 0) {
      char* p = reinterpret_cast<char*>(s + (upto - len));
      if (J.section == 0) {
        p += fixed4_put(P, p);
      } else {
        p += fixed4_put(u_x, p);
        *p++ = ' ';
        p += fixed4_put(u_y, p);
        *p++ = ' '; *p++ = '0'; *p++ = '.';
      }
      *p = '\n';
    }
    __syncthreads();
    if (row && total > 0 && at >= 0 && at + total <= J.cap) {
      unsigned char* g = J.out + at;
      int head = (4 - al) & 3;
      if (head > total) head = total;
      const int words = (total - head) / 4, tail = head + 4 * words;
      if (lane < head) g[lane] = s[lane];
      for (int k = lane; k < words; k += 64)
        *reinterpret_cast<unsigned*>(g + head + 4 * k) = *reinterpret_cast<const unsigned*>(s + head + 4 * k);
      if (tail + lane < total) g[tail + lane] = s[tail + lane];
    }
    __syncthreads();   // (the next row's text goes to the same place)
  }
}

// what the count pass and the scan leave on the host
struct DensPlan {
  std::vector<long long> rowoff;   // [2 * ly + 1] where every file row of the Pressure, then of the VecVelocity section begins
                                   // in the body; the last entry is the body's length
  std::vector<double> prow;        // [lx]
  long refused = 0;
  long long section_bytes(int s, int ly) const { return rowoff[(size_t)(s + 1) * ly] - rowoff[(size_t)s * ly]; }
};

int dens_job(lbmdem_handle* h, const char* who, DensJob* J) {
  RC_TRY(whole_handle(h, who));
  const LatticeView& L = h->L;
  *J = DensJob{};
  J->f = h->f[h->fcur];
  J->obst = reader_obst(h);
  J->L = L;
  J->L.gate = nullptr;
  J->rho_moy = (real)h->cfg.phys.rho_moy;
  J->nxb = (L.lx + DN_BX - 1) / DN_BX;
  J->ncell = (long long)L.ly * J->nxb;
  return LBMDEM_OK;
}

// count pass and scan; J.cells is the scan afterwards (in memory of `mem`, the caller's pool: it outlives this function)
int dens_plan(lbmdem_handle* h, DensJob& J, MemPool& mem, DensPlan* P) {
  const LatticeView& L = J.L;
  const size_t nall = 2 * (size_t)J.ncell + 1;
  MemPool scratch;
  long long *cells = nullptr, *offsets = nullptr;
  double* prow = nullptr;
  unsigned* refused = nullptr;
  void* tmp = nullptr;
  HIP_TRY(mem.dev(&cells, nall));
  HIP_TRY(mem.dev(&offsets, nall));
  HIP_TRY(scratch.dev(&prow, (size_t)L.lx));
  HIP_TRY(scratch.dev(&refused, 1));
  HIP_TRY(hipMemsetAsync(cells + nall - 1, 0, sizeof(long long), h->stream));
  HIP_TRY(hipMemsetAsync(prow, 0, sizeof(double) * L.lx, h->stream));
  HIP_TRY(hipMemsetAsync(refused, 0, sizeof(unsigned), h->stream));
  J.cells = cells;
  J.prow = prow;
  J.refused = refused;
  hipLaunchKernelGGL(k_dens_count, dim3(J.nxb, (L.ly + DN_TY - 1) / DN_TY), dim3(256), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cells, offsets, (int)nall, h->stream));
  HIP_TRY(scratch.dev(&tmp, tmp_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cells, offsets, (int)nall, h->stream));
  P->rowoff.assign(2 * (size_t)L.ly + 1, 0);
  P->prow.assign(L.lx, 0.);
  unsigned bad = 0;
  // every file row's first cell: the cells of both sections lie row after row, nxb apart
  HIP_TRY(hipMemcpy2DAsync(P->rowoff.data(), sizeof(long long), offsets, sizeof(long long) * J.nxb, sizeof(long long),
                           2 * (size_t)L.ly, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&P->rowoff[2 * (size_t)L.ly], offsets + nall - 1, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(P->prow.data(), prow, sizeof(double) * L.lx, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&bad, refused, sizeof bad, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  P->refused = (long)bad;
  J.cells = offsets;
  J.prow = nullptr;
  J.refused = nullptr;
  return LBMDEM_OK;
}

constexpr size_t DENS_STAGING_DEFAULT = (size_t)64 << 20;

// The body, band after band, to put(text, bytes). A section's bands hold as many whole file rows as the budget has room for
// the section's longest row -- at least one: the budget is never less than the longest row of the file.
template <class Put>
int dens_emit(lbmdem_handle* h, DensJob J, const DensPlan& P, Put put, long* bands) {
  const int ly = J.L.ly;
  long long longest[2] = {1, 1};
  for (int s = 0; s < 2; ++s)
    for (int y = 0; y < ly; ++y) {
      const long long b = P.rowoff[(size_t)s * ly + y + 1] - P.rowoff[(size_t)s * ly + y];
      if (b > longest[s]) longest[s] = b;
    }
  long long budget = (long long)(h->dens_budget ? h->dens_budget : DENS_STAGING_DEFAULT);
  if (budget < longest[0]) budget = longest[0];
  if (budget < longest[1]) budget = longest[1];
  int rows[2];
  long long need = 1;
  for (int s = 0; s < 2; ++s) {
    const long long k = budget / longest[s];
    rows[s] = (int)(k < ly ? k : ly);
    for (int y0 = 0; y0 < ly; y0 += rows[s]) {
      const int y1 = y0 + rows[s] < ly ? y0 + rows[s] : ly;
      const long long b = P.rowoff[(size_t)s * ly + y1] - P.rowoff[(size_t)s * ly + y0];
      if (b > need) need = b;
    }
  }
  MemPool scratch;
  unsigned char* staging = nullptr;
  char* pinned = nullptr;
  HIP_TRY(scratch.dev(&staging, (size_t)need));
  HIP_TRY(scratch.pinned(&pinned, (size_t)need));
  J.out = staging;
  *bands = 0;
  for (int s = 0; s < 2; ++s)
    for (int y0 = 0; y0 < ly; y0 += rows[s]) {
      const int y1 = y0 + rows[s] < ly ? y0 + rows[s] : ly;
      J.section = s; J.y0 = y0; J.y1 = y1;
      J.base = P.rowoff[(size_t)s * ly + y0];
      J.cap = P.rowoff[(size_t)s * ly + y1] - J.base;   // (<= need)
      ++*bands;
      if (J.cap == 0) continue;
      hipLaunchKernelGGL(k_dens_emit, dim3(J.nxb, (y1 - 1) / DN_TY - y0 / DN_TY + 1), dim3(256), 0, h->stream, J);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(pinned, staging, (size_t)J.cap, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      put(pinned, (size_t)J.cap);
    }
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

// where text goes: a file, memory (what does not fit is counted, not stored), or nowhere (mem == nullptr: counted only)
struct Sink {
  FILE* fp = nullptr;
  char* mem = nullptr;
  size_t cap = 0, at = 0;
  void put(const char* s, size_t n) {
    if (fp) fwrite(s, 1, n, fp);
    else if (mem && at + n <= cap) memcpy(mem + at, s, n);
    at += n;
  }
  void print(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    va_list ap;
    va_start(ap, fmt);
    if (fp) {
      const int n = vfprintf(fp, fmt, ap);
      if (n > 0) at += (size_t)n;
    } else {
      char tmp[512];
      const int n = vsnprintf(tmp, sizeof tmp, fmt, ap);
      if (n > 0) put(tmp, (size_t)n < sizeof tmp ? (size_t)n : sizeof tmp - 1);
    }
    va_end(ap);
  }
};

// main.c:498-520
void put_head(Sink& S, int lx, int ly, double t) {
  const double pasxyz = 1. / lx;
  S.print("# vtk DataFile Version 2.0\n");
  S.print("Outfile domain LB t: %e\n", t);
  S.print("ASCII\n");
  S.print("DATASET RECTILINEAR_GRID\n");
  S.print("DIMENSIONS %d %d 1\n", lx, ly);
  S.print("X_COORDINATES %d float\n", lx);
  for (int i = 0; i <= lx - 1; i++) S.print("%e ", (float)i * pasxyz);
  S.print("\n");
  S.print("Y_COORDINATES %d float\n", ly);
  for (int i = 0; i <= ly - 1; i++) S.print("%e ", (float)i * pasxyz);
  S.print("\n");
  S.print("Z_COORDINATES 1 float\n");
  S.print("0\n");
  S.print("POINT_DATA %d\n", lx * ly);
  S.print("SCALARS Pressure float 1\n");
  S.print("LOOKUP_TABLE default\n");
}
const char* const VELOCITY_HEAD = "VECTORS VecVelocity float\n";

// main.c:522-562, the reference's loops and format strings over host arrays f[lx][ly][9], obst[lx][ly]; `head`: the line
// between the two sections. bytes2: what each section took.
void host_body(Sink& S, Sink* press, bool head, int lx, int ly, double rho_moy, const double* f, const int* obst, long* bytes2) {
  const double pasxyz = 1. / lx;
  int x, y, i;
  double P, u_x, u_y;
  const size_t at0 = S.at;
  for (y = 0; y < ly; y++) {
    for (x = 0; x < lx; x++) {
      const double* fn = f + ((size_t)x * ly + y) * 9;
      P = 0.;
      for (i = 0; i < 9; i++) P += fn[i];
      P = (1. / 3.) * rho_moy * (P - 1.);
      if (obst[(size_t)x * ly + y] < 0) {
        S.print("%.4lf\n", P);
        if (y == 2 && press) press->print("%le %le\n", x * pasxyz, P);
      } else {
        S.print("%.4lf\n", 0.);
        if (y == 2 && press) press->print("%le %le\n", x * pasxyz, 0.0);
      }
    }
  }
  const size_t at1 = S.at;
  if (head) S.print("%s", VELOCITY_HEAD);
  const size_t at2 = S.at;
  for (y = 0; y < ly; y++) {
    for (x = 0; x < lx; x++) {
      const double* fn = f + ((size_t)x * ly + y) * 9;
      u_x = 0.;
      u_y = 0.;
      for (i = 0; i < 9; i++) {
        u_x += fn[i] * EXq(i);
        u_y += fn[i] * EYq(i);
      }
      if (obst[(size_t)x * ly + y] < 0) S.print("%.4lf %.4lf 0.\n", u_x, u_y);
      else S.print("%.4lf %.4lf 0.\n", 0., 0.);
    }
  }
  if (bytes2) { bytes2[0] = (long)(at1 - at0); bytes2[1] = (long)(S.at - at2); }
}

// the two files of one call, opened together (unlike the reference, fopen is checked)
struct DensFiles {
  OutFile vtk, press;
  int open(const char* dir, int nfile) {
    RC_TRY(vtk.open("w", dir, "densities%.6i.vtk", nfile));
    return press.open("w", dir, "pressure_base%.6i.dat", nfile);
  }
  int close() {   // (one text for the pair)
    const bool bad_vtk = vtk.finish(), bad_press = press.finish();
    if (bad_vtk || bad_press) return fail(LBMDEM_EINVAL, "writing '%s' or '%s' failed", vtk.path, press.path);
    return LBMDEM_OK;
  }
};

int write_host(DensFiles& F, int lx, int ly, double t, double rho_moy, const double* f, const int* obst, long* bytes2) {
  Sink S, Sp;
  S.fp = F.vtk.fp;
  Sp.fp = F.press.fp;
  put_head(S, lx, ly, t);
  host_body(S, &Sp, true, lx, ly, rho_moy, f, obst, bytes2);
  return F.close();
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_densities_host(const char* dir, int nfile, int lx, int ly, double t, double rho_moy, const double* f_aos,
                                const int* obst) {
  if (!f_aos || !obst || lx < 1 || ly < 1) return fail(LBMDEM_EINVAL, "bad lbmdem_write_densities_host arguments");
  DensFiles F;
  RC_TRY(F.open(dir, nfile));
  return write_host(F, lx, ly, t, rho_moy, f_aos, obst, nullptr);
}

int lbmdem_format_fixed4(const double* v, long n, char* out, long cap, long* bytes) {
  if (!bytes || n < 0 || cap < 0 || (n > 0 && !v) || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "bad lbmdem_format_fixed4 arguments");
  long need = 0;
  for (long k = 0; k < n; ++k) {
    if (!fixed4_ok(v[k])) return fail(LBMDEM_EINVAL, "lbmdem_format_fixed4: value %ld is not finite or not below 1e9", k);
    need += fixed4_len(v[k]) + 1;
  }
  *bytes = need;
  if (cap < need) return fail(LBMDEM_EINVAL, "lbmdem_format_fixed4: the text has %ld bytes, the buffer holds %ld", need, cap);
  char* p = out;
  for (long k = 0; k < n; ++k) {
    p += fixed4_put(v[k], p);
    *p++ = '\n';
  }
  return LBMDEM_OK;
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_write_densities(lbmdem_handle* h, const char*, int) { SP_REFUSE(h, "write_densities"); }
int lbmdem_download_densities_text(lbmdem_handle* h, char*, size_t, size_t*) { SP_REFUSE(h, "write_densities"); }
int lbmdem_set_densities_staging(lbmdem_handle* h, size_t) { SP_REFUSE(h, "write_densities"); }
int lbmdem_densities_stats(lbmdem_handle* h, long*) { SP_REFUSE(h, "write_densities"); }
#else

int lbmdem_set_densities_staging(lbmdem_handle* h, size_t bytes) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  h->dens_budget = bytes;
  return LBMDEM_OK;
}

int lbmdem_densities_stats(lbmdem_handle* h, long* counts4) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (!counts4) return fail(LBMDEM_EINVAL, "null buffer");
  for (int k = 0; k < 4; ++k) counts4[k] = h->dens_stats[k];
  return LBMDEM_OK;
}

int lbmdem_write_densities(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  DensJob J;
  RC_TRY(dens_job(h, "lbmdem_write_densities", &J));
  const int lx = J.L.lx, ly = J.L.ly;
  DensFiles F;
  RC_TRY(F.open(dir, nfile));
  MemPool scratch;   // (the plan's cell offsets live here until the body is out)
  DensPlan P;
  RC_TRY(dens_plan(h, J, scratch, &P));
  if (P.refused > 0) {   // the reference's own loops print what the device does not: nan, inf, ten digits and more
    std::vector<double> f((size_t)lx * ly * 9);
    std::vector<int> obst((size_t)lx * ly);
    RC_TRY(lbmdem_download_f(h, f.data()));
    RC_TRY(lbmdem_download_obst(h, obst.data()));
    long b[2] = {0, 0};
    RC_TRY(write_host(F, lx, ly, h->cfg.phys.t, h->cfg.phys.rho_moy, f.data(), obst.data(), b));
    h->dens_stats[0] = b[0]; h->dens_stats[1] = b[1]; h->dens_stats[2] = 0; h->dens_stats[3] = P.refused;
    return LBMDEM_OK;
  }
  Sink S, Sp;
  S.fp = F.vtk.fp;
  Sp.fp = F.press.fp;
  put_head(S, lx, ly, h->cfg.phys.t);
  const long long pbytes = P.section_bytes(0, ly);
  long long done = 0;
  long bands = 0;
  RC_TRY(dens_emit(h, J, P, [&](const char* s, size_t n) {
    if (done == pbytes) S.print("%s", VELOCITY_HEAD);   // (a band never spans the two sections)
    S.put(s, n);
    done += (long long)n;
  }, &bands));
  if (ly > 2) {   // main.c:531-533, 536-538
    const double pasxyz = 1. / lx;
    for (int x = 0; x < lx; x++) Sp.print("%le %le\n", x * pasxyz, P.prow[x]);
  }
  RC_TRY(F.close());
  h->dens_stats[0] = (long)pbytes; h->dens_stats[1] = (long)P.section_bytes(1, ly); h->dens_stats[2] = bands; h->dens_stats[3] = 0;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_densities_text(lbmdem_handle* h, char* out, size_t cap, size_t* bytes) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!bytes || (cap > 0 && !out)) return fail(LBMDEM_EINVAL, "null buffer");
  DensJob J;
  RC_TRY(dens_job(h, "lbmdem_download_densities_text", &J));
  const int lx = J.L.lx, ly = J.L.ly;
  MemPool scratch;   // (the plan's cell offsets live here until the body is out)
  DensPlan P;
  RC_TRY(dens_plan(h, J, scratch, &P));
  if (P.refused > 0) {
    std::vector<double> f((size_t)lx * ly * 9);
    std::vector<int> obst((size_t)lx * ly);
    RC_TRY(lbmdem_download_f(h, f.data()));
    RC_TRY(lbmdem_download_obst(h, obst.data()));
    Sink S;
    S.mem = out; S.cap = cap;
    long b[2] = {0, 0};
    host_body(S, nullptr, false, lx, ly, h->cfg.phys.rho_moy, f.data(), obst.data(), b);
    *bytes = S.at;
    h->dens_stats[0] = b[0]; h->dens_stats[1] = b[1]; h->dens_stats[2] = 0; h->dens_stats[3] = P.refused;
    if (S.at > cap) return fail(LBMDEM_EINVAL, "lbmdem_download_densities_text: the text has %zu bytes, the buffer holds %zu", S.at, cap);
    return LBMDEM_OK;
  }
  const size_t total = (size_t)P.rowoff[2 * (size_t)ly];
  *bytes = total;
  if (cap < total) return fail(LBMDEM_EINVAL, "lbmdem_download_densities_text: the text has %zu bytes, the buffer holds %zu", total, cap);
  size_t at = 0;
  long bands = 0;
  RC_TRY(dens_emit(h, J, P, [&](const char* s, size_t n) { memcpy(out + at, s, n); at += n; }, &bands));
  h->dens_stats[0] = (long)P.section_bytes(0, ly); h->dens_stats[1] = (long)P.section_bytes(1, ly); h->dens_stats[2] = bands; h->dens_stats[3] = 0;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
