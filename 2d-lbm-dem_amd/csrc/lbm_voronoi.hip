// lbm_voronoi.hip -- how much space a grain has: the radical (power, Laguerre) tessellation of the discs inside the four walls, per
// grain its cell's area, perimeter, local solid fraction and topological neighbour count, and the cells' faces -- the Delaunay graph
// and the wall faces -- as CSR (lbmdem_voronoi_compute, lbmdem_download_voronoi_grains, lbmdem_voronoi_grains_device,
// lbmdem_download_voronoi_faces, lbmdem_write_voronoi, lbmdem_set_voronoi_output, lbmdem_write_voronoi_files; include/lbmdem_hip.h
// has the contract in full). A cell is the box clipped by the radical line of every neighbour of lbm_structure.hip's list in list
// order: a chain of IEEE double operations in a stated order that one lane walks serially. The census is integers; no
// floating-point atomics anywhere. Nothing here is on the step path: the kernels only read the structure stage and the kinematics
// and write to the handle's VoronoiStage, and nothing is allocated or launched before the first compute.
//
// On the handle's stream:
//   k_vo_cells   one lane per grain, 64 lanes per workgroup. A lane keeps its polygon of at most 32 vertices twice (the one it
//                clips and the one it makes) in an LDS slice of its own, vertex k of lane l at [k][l]: lanes that are at the same
//                vertex touch neighbouring banks, and a clip costs no global traffic beyond the partner's x, y, r, which are
//                fetched one neighbour ahead. 80 KiB per workgroup, two workgroups per CU: at 50 000 grains there are three
//                workgroups per CU to run, so the occupancy the LDS leaves is no limit, and the latency of every vertex access
//                is (LABBOOK.md has the time). A partner whose line provably passes outside the circle around the cell (h beyond
//                the cell's largest |v - x_i| times |x_j - x_i|, with a margin that covers the rounding) is skipped without a
//                walk: such a line cuts nothing, and a line that cuts nothing leaves the polygon as it was. The measures, the
//                faces into rows [k][n], the face count; the census by wavefront sums and one integer atomic per word;
//   a scan       foff[n + 1] over the face counts by index;
//   k_vo_emit    one lane per grain copies its row into the CSR.
// No workgroup waits for another; every loop has a bound.
// Double-precision library only: the entry points that take a handle refuse in the float build; the host-only formatter exists in
// both.
// Front end, as every export's: whole_handle() and SP_REFUSE() (lbmdem_handle.h) for the refusals, MemPool::grow (lbm_mem.h) for
// the scratch kept on the handle, OutFile (lbm_outfile.h) for the files.
#include "lbm_outfile.h"

#include <errno.h>
#include <float.h>
#include <limits.h>
#include <math.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include <hipcub/hipcub.hpp>
#endif

namespace {

constexpr int VOR_MAXV = LBMDEM_VOR_MAXV;
constexpr double VOR_PI = 3.141592653589793;   // (lbm_structure.hip's ST_PI)

bool vo_finite(double v) { return v - v == 0.; }

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int VO_LANES = 64;      // grains of a workgroup of the cell pass: one wavefront
constexpr int VO_THREADS = 256;   // the emit
// VoronoiStage::words: the census
enum : int { VO_CELLS = 0, VO_COMPLETE, VO_EMPTY, VO_OVERFLOW, VO_NONFINITE, VO_GFACES, VO_WFACES, VO_MAXFACES, VO_WORDS };

struct VoJob {
  const double *x, *y, *r;   // the centres lbmdem_download_grain_table shows, the radii
  const int *off, *nbr;      // the structure stage's list
  int n;
  double gx, dx, by, hy;     // the walls where they stand: Mgx, Mdx, Mby, Mhy
  double rcut, rmax;
  double *area, *perimeter, *phi, *R2;
  int *faces, *walls, *nverts, *flags;
  int *nf, *foff;            // [n + 1] both
  int* rsrc;
  double* rlen;
  int* fsrc;
  double* flen;
  unsigned long long* words;
};

__device__ __forceinline__ bool vo_dfinite(double v) { return v - v == 0.; }

// the reach with one more vertex at squared distance w; a vertex that is no finite point puts it out of reach of the skip
__device__ __forceinline__ double vo_reach(double reach2, double w) {
  if (!(w <= DBL_MAX)) return INFINITY;
  return w > reach2 ? w : reach2;
}

__device__ __forceinline__ unsigned long long vo_wave_sum(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);   // (every lane of the wavefront is here)
  return v;
}

__global__ __launch_bounds__(VO_LANES) void k_vo_cells(const VoJob J) {
  __shared__ double px[2][VOR_MAXV][VO_LANES], py[2][VOR_MAXV][VO_LANES];
  __shared__ int ps[2][VOR_MAXV][VO_LANES];
  const int lane = threadIdx.x, n = J.n;
  const int i = blockIdx.x * VO_LANES + lane;
  const bool mine = i < n;
  double xi = 0., yi = 0., ri = 0.;
  int m = 0, cur = 0, flags = 0;
  int k0 = 0, k1 = 0;
  if (mine) {
    xi = J.x[i]; yi = J.y[i]; ri = J.r[i];
    if (vo_dfinite(xi) && vo_dfinite(yi)) {
      px[0][0][lane] = J.gx; py[0][0][lane] = J.by; ps[0][0][lane] = -1;
      px[0][1][lane] = J.dx; py[0][1][lane] = J.by; ps[0][1][lane] = -2;
      px[0][2][lane] = J.dx; py[0][2][lane] = J.hy; ps[0][2][lane] = -3;
      px[0][3][lane] = J.gx; py[0][3][lane] = J.hy; ps[0][3][lane] = -4;
      m = 4;
      k0 = J.off[i]; k1 = J.off[i + 1];
    } else {
      flags |= LBMDEM_VOR_NONFINITE;
    }
  }
  // the largest |v - x_i|^2 over the polygon, for the skip alone (the measure R2 is made from the final polygon below)
  double reach2 = 0.;
  for (int v = 0; v < m; ++v) {
    const double ax = px[0][v][lane] - xi, ay = py[0][v][lane] - yi;
    reach2 = vo_reach(reach2, ax * ax + ay * ay);
  }
  // the partner of the coming round, fetched a round ahead
  int jn = -1;
  double xn = 0., yn = 0., rn = 0.;
  if (k0 < k1) {
    jn = J.nbr[k0];
    if (jn >= 0 && jn < n) { xn = J.x[jn]; yn = J.y[jn]; rn = J.r[jn]; }
  }
  for (int k = k0; k < k1 && m > 0; ++k) {
    const int j = jn;
    const double xj = xn, yj = yn, rj = rn;
    if (k + 1 < k1) {
      jn = J.nbr[k + 1];
      if (jn >= 0 && jn < n) { xn = J.x[jn]; yn = J.y[jn]; rn = J.r[jn]; }
    }
    if (j < 0 || j >= n) continue;   // (never: the list holds grains)
    const double dx = xj - xi, dy = yj - yi;
    const double d2 = dx * dx + dy * dy;
    if (!(d2 > 0.)) continue;
    const double h = 0.5 * ((d2 + ri * ri) - rj * rj);
    // s <= |v - x_i| |x_j - x_i| - h for every vertex: beyond that the line cuts nothing (never with a reach of infinity or a NaN)
    if (h > 0. && h * h > 1.000001 * (reach2 * d2)) continue;
    const int nxt = cur ^ 1;
    int q = 0;
    bool cut = false;
    double grown = 0.;
    double ax = px[cur][0][lane], ay = py[cur][0][lane];
    int as = ps[cur][0][lane];
    double sa = ((ax - xi) * dx + (ay - yi) * dy) - h;
    const double x0 = ax, y0 = ay, s0 = sa;
    for (int v = 0; v < m; ++v) {
      double bx = x0, by = y0, sb = s0;
      int bs = 0;
      if (v + 1 < m) {
        bx = px[cur][v + 1][lane]; by = py[cur][v + 1][lane]; bs = ps[cur][v + 1][lane];
        sb = ((bx - xi) * dx + (by - yi) * dy) - h;
      }
      const bool ina = sa <= 0., inb = sb <= 0.;
      if (ina) {
        if (q < VOR_MAXV) { px[nxt][q][lane] = ax; py[nxt][q][lane] = ay; ps[nxt][q][lane] = as; }
        ++q;
        const double ux = ax - xi, uy = ay - yi;
        grown = vo_reach(grown, ux * ux + uy * uy);
      } else {
        cut = true;
      }
      if (ina != inb) {
        const double t = sa / (sa - sb);
        const double cx = ax + t * (bx - ax), cy = ay + t * (by - ay);
        if (q < VOR_MAXV) { px[nxt][q][lane] = cx; py[nxt][q][lane] = cy; ps[nxt][q][lane] = ina ? j : as; }
        ++q;
        const double ux = cx - xi, uy = cy - yi;
        grown = vo_reach(grown, ux * ux + uy * uy);
      }
      ax = bx; ay = by; sa = sb; as = bs;
    }
    if (!cut) continue;   // the polygon as it was
    if (q > VOR_MAXV) {
      m = 0;
      flags |= LBMDEM_VOR_OVERFLOW;
    } else {
      m = q; cur = nxt; reach2 = grown;
    }
  }
  // the measures, one walk from +0.0
  double A2 = 0., per = 0., R2 = 0.;
  int faces = 0, walls = 0, nf = 0, wf = 0;
  if (m > 0) {
    double ax = px[cur][0][lane], ay = py[cur][0][lane];
    int as = ps[cur][0][lane];
    const double x0 = ax, y0 = ay;
    for (int v = 0; v < m; ++v) {
      double bx = x0, by = y0;
      int bs = 0;
      if (v + 1 < m) { bx = px[cur][v + 1][lane]; by = py[cur][v + 1][lane]; bs = ps[cur][v + 1][lane]; }
      const double ux = ax - xi, uy = ay - yi, wx = bx - xi, wy = by - yi;
      A2 += ux * wy - wx * uy;
      const double ex = bx - ax, ey = by - ay;
      const double len = sqrt(ex * ex + ey * ey);
      per += len;
      const double q = ux * ux + uy * uy;
      if (q > R2) R2 = q;
      if (ax != bx || ay != by) {
        J.rsrc[(size_t)nf * n + i] = as;
        J.rlen[(size_t)nf * n + i] = len;
        ++nf;
        if (as >= 0) ++faces;
        else { walls |= 1 << (-as - 1); ++wf; }
      }
      ax = bx; ay = by; as = bs;
    }
  }
  const double area = 0.5 * A2;
  const double phi = area > 0. ? ((VOR_PI * ri) * ri) / area : 0.;
  const double bound = 0.5 * (J.rcut + (ri * ri - J.rmax * J.rmax) / J.rcut);
  if (m > 0 && bound > 0. && R2 <= bound * bound) flags |= LBMDEM_VOR_COMPLETE;
  if (mine && m == 0 && !(flags & LBMDEM_VOR_OVERFLOW)) flags |= LBMDEM_VOR_EMPTY;
  if (mine) {
    J.area[i] = area; J.perimeter[i] = per; J.phi[i] = phi; J.R2[i] = R2;
    J.faces[i] = faces; J.walls[i] = walls; J.nverts[i] = m; J.flags[i] = flags;
    J.nf[i] = nf;
    if (i == 0) J.nf[n] = 0;   // the scan's last item
  }
  // the census: sums of the wavefront, then one integer atomic per word
  const unsigned long long c_area = vo_wave_sum(mine && area > 0. ? 1ull : 0ull);
  const unsigned long long c_comp = vo_wave_sum((flags & LBMDEM_VOR_COMPLETE) ? 1ull : 0ull);
  const unsigned long long c_empty = vo_wave_sum((flags & LBMDEM_VOR_EMPTY) ? 1ull : 0ull);
  const unsigned long long c_over = vo_wave_sum((flags & LBMDEM_VOR_OVERFLOW) ? 1ull : 0ull);
  const unsigned long long c_bad = vo_wave_sum((flags & LBMDEM_VOR_NONFINITE) ? 1ull : 0ull);
  const unsigned long long c_gf = vo_wave_sum((unsigned long long)faces);
  const unsigned long long c_wf = vo_wave_sum((unsigned long long)wf);
  unsigned long long c_max = (unsigned long long)faces;
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(c_max, s);
    c_max = o > c_max ? o : c_max;
  }
  if (lane == 0) {
    if (c_area) atomicAdd(&J.words[VO_CELLS], c_area);
    if (c_comp) atomicAdd(&J.words[VO_COMPLETE], c_comp);
    if (c_empty) atomicAdd(&J.words[VO_EMPTY], c_empty);
    if (c_over) atomicAdd(&J.words[VO_OVERFLOW], c_over);
    if (c_bad) atomicAdd(&J.words[VO_NONFINITE], c_bad);
    if (c_gf) atomicAdd(&J.words[VO_GFACES], c_gf);
    if (c_wf) atomicAdd(&J.words[VO_WFACES], c_wf);
    atomicMax(&J.words[VO_MAXFACES], c_max);
  }
}

__global__ __launch_bounds__(VO_THREADS) void k_vo_emit(const VoJob J) {
  const int i = blockIdx.x * VO_THREADS + threadIdx.x;
  if (i >= J.n) return;
  const int f0 = J.foff[i];
  int nf = J.foff[i + 1] - f0;
  if (nf > VOR_MAXV) nf = VOR_MAXV;   // (never: a cell has at most that many vertices)
  for (int k = 0; k < nf; ++k) {
    J.fsrc[f0 + k] = J.rsrc[(size_t)k * J.n + i];
    J.flen[f0 + k] = J.rlen[(size_t)k * J.n + i];
  }
}

int vo_blocks(long items, int threads) { return (int)((items + threads - 1) / threads); }

// what depends on n, once
int voronoi_stage(lbmdem_handle* h) {
  auto& V = h->vo;
  const size_t n = (size_t)h->n;
  if (V.words) return LBMDEM_OK;
  HIP_TRY(h->mem.dev(&V.dbl, 4 * n));
  HIP_TRY(h->mem.dev(&V.ints, 6 * n + 2));
  HIP_TRY(h->mem.dev(&V.rsrc, (size_t)VOR_MAXV * n));
  HIP_TRY(h->mem.dev(&V.rlen, (size_t)VOR_MAXV * n));
  size_t b = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int*)nullptr, (int*)nullptr, (int)n + 1, h->stream));
  HIP_TRY(h->mem.grow(&V.tmp, &V.tmp_bytes, (long)b));
  HIP_TRY(h->mem.dev(&V.words, (size_t)VO_WORDS));   // (last: the mark of a finished allocation)
  return LBMDEM_OK;
}

// lbm_structure.hip keeps rcut*rcut, the last edge of its table, and not rcut. Squaring is one-to-one on the doubles whose
// square is a normal number (neighbouring doubles have squares at least 1.41 ulp apart, and rounding cannot merge those), so rcut
// is the one double whose square rounds to that edge: the root, or a neighbour of it.
int vo_rcut_of(double rc2, double* rcut) {
  if (!(rc2 >= DBL_MIN) || !(rc2 <= DBL_MAX)) return 1;
  double c = sqrt(rc2);
  for (int step = 0; step < 4 && c * c > rc2; ++step) c = nextafter(c, 0.);
  for (int step = 0; step < 4 && c * c < rc2; ++step) c = nextafter(c, DBL_MAX);
  if (c * c != rc2) return 1;
  *rcut = c;
  return 0;
}

int voronoi_ready(const lbmdem_handle* h, const char* who) {
  RC_TRY(whole_handle(h, who));
  const auto& V = h->vo;
  if (!V.valid || V.seq != h->substep_seq || V.moved != h->grains_moved || V.walls != h->walls_moved)
    return fail(LBMDEM_EINVAL, "%s: no lbmdem_voronoi_compute has been made for the grains where they are now", who);
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_voronoi_files(const char* dir, int nfile, int n, const double* area, const double* perimeter, const double* phi,
                               const int* faces, const int* walls, const int* nverts, const int* flags, double rcut,
                               const long* counts8, double t, double W, double H) try {
  if (n < 1 || !area || !perimeter || !phi || !faces || !walls || !nverts || !flags || !counts8)
    return fail(LBMDEM_EINVAL, "bad lbmdem_write_voronoi_files arguments");
  if (!(rcut > 0) || !vo_finite(rcut)) return fail(LBMDEM_EINVAL, "lbmdem_write_voronoi_files: rcut must be finite and > 0 (%le)", rcut);
  for (int i = 0; i < n; ++i)
    if (nverts[i] < 0 || nverts[i] > VOR_MAXV || faces[i] < 0 || faces[i] > nverts[i])
      return fail(LBMDEM_EINVAL, "lbmdem_write_voronoi_files: grain %d has %d faces on %d vertices, a cell has at most %d", i, faces[i],
                  nverts[i], VOR_MAXV);
  OutFile F;
  RC_TRY(F.open("w", dir, "voronoi%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# rcut %le\n", rcut);
  fprintf(fp, "# i area perimeter phi faces walls nverts flags\n");
  for (int i = 0; i < n; ++i)
    fprintf(fp, "%d %le %le %le %d %d %d %d\n", i, area[i], perimeter[i], phi[i], faces[i], walls[i], nverts[i], flags[i]);
  RC_TRY(F.close());
  // serial sums by index
  double sum_area = 0., sum_phi = 0., sum_faces = 0.;
  long with = 0;
  for (int i = 0; i < n; ++i) {
    sum_area += area[i];
    if ((flags[i] & LBMDEM_VOR_COMPLETE) && area[i] > 0) { sum_phi += phi[i]; sum_faces += (double)faces[i]; ++with; }
  }
  const double mean_phi = with > 0 ? sum_phi / (double)with : 0.;
  const double mean_faces = with > 0 ? sum_faces / (double)with : 0.;
  RC_TRY(F.open("a", dir, "voronoi.data"));
  fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0)
    fprintf(fp, "# t cells complete empty overflowed nonfinite_grains grain_faces wall_faces max_faces sum_area box_area mean_phi "
                "mean_faces\n");
  fprintf(fp, "%le", t);
  for (int k = 0; k < 8; ++k) fprintf(fp, " %ld", counts8[k]);
  fprintf(fp, " %le %le %le %le\n", sum_area, W * H, mean_phi, mean_faces);
  return F.close();
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_voronoi_compute(lbmdem_handle* h, long*) { SP_REFUSE(h, "the Voronoi analysis"); }
int lbmdem_download_voronoi_grains(lbmdem_handle* h, double*, double*, double*, double*, int*, int*, int*, int*) { SP_REFUSE(h, "the Voronoi analysis"); }
int lbmdem_voronoi_grains_device(lbmdem_handle* h, const double**, const double**, const double**, const double**, const int**, const int**, const int**, const int**) { SP_REFUSE(h, "the Voronoi analysis"); }
int lbmdem_download_voronoi_faces(lbmdem_handle* h, int*, int*, double*, long, long*) { SP_REFUSE(h, "the Voronoi analysis"); }
int lbmdem_write_voronoi(lbmdem_handle* h, const char*, int, double) { SP_REFUSE(h, "the Voronoi analysis"); }
int lbmdem_set_voronoi_output(lbmdem_handle* h, int, double) { SP_REFUSE(h, "the Voronoi analysis"); }
#else

int lbmdem_voronoi_compute(lbmdem_handle* h, long* counts8) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts8) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_voronoi_compute"));
  const auto& S = h->st;
  auto& V = h->vo;
  V.valid = false;
  if (!S.valid || S.seq != h->substep_seq || S.moved != h->grains_moved)
    return fail(LBMDEM_EINVAL, "lbmdem_voronoi_compute: no lbmdem_structure_compute has been made for the grains where they are now");
  if (!S.listed)
    return fail(LBMDEM_EINVAL, "lbmdem_voronoi_compute: the last lbmdem_structure_compute had max_entries == 0: counts and "
                               "histogram only, and the cells need its neighbour list");
  const hipStream_t st = h->stream;
  double rc2 = 0., rcut = 0.;
  HIP_TRY(hipMemcpyAsync(&rc2, S.e2 + S.nbins, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (vo_rcut_of(rc2, &rcut))
    return fail(LBMDEM_EINVAL, "lbmdem_voronoi_compute: the square of the rcut of the last lbmdem_structure_compute is no normal "
                               "number (%le)", rc2);
  RC_TRY(voronoi_stage(h));
  const int n = h->n;
  const size_t N = (size_t)n;
  const lbmdem_config& c = h->cfg;
  VoJob J{};
  J.x = h->kin[h->kcur].x1; J.y = h->kin[h->kcur].x2; J.r = h->r;
  J.off = S.ints + 2 * N + 1; J.nbr = S.nbr;
  J.n = n;
  J.gx = c.Mgx; J.dx = c.Mdx; J.by = c.Mby; J.hy = c.Mhy;
  J.rcut = rcut; J.rmax = h->rmax;
  J.area = V.dbl; J.perimeter = V.dbl + N; J.phi = V.dbl + 2 * N; J.R2 = V.dbl + 3 * N;
  J.faces = V.ints; J.walls = V.ints + N; J.nverts = V.ints + 2 * N; J.flags = V.ints + 3 * N;
  J.nf = V.ints + 4 * N; J.foff = V.ints + 5 * N + 1;
  J.rsrc = V.rsrc; J.rlen = V.rlen;
  J.words = V.words;
  HIP_TRY(hipMemsetAsync(V.words, 0, sizeof(unsigned long long) * VO_WORDS, st));
  hipLaunchKernelGGL(k_vo_cells, dim3(vo_blocks(n, VO_LANES)), dim3(VO_LANES), 0, st, J);
  HIP_TRY(hipGetLastError());
  size_t bytes = (size_t)V.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(V.tmp, bytes, J.nf, J.foff, n + 1, st));
  unsigned long long w[VO_WORDS] = {};
  HIP_TRY(hipMemcpyAsync(w, V.words, sizeof w, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const long nfaces = (long)(w[VO_GFACES] + w[VO_WFACES]);
  if (nfaces > 0) {
    HIP_TRY(h->mem.grow(&V.fsrc, &V.fsrc_cap, nfaces + nfaces / 4 + 64));
    HIP_TRY(h->mem.grow(&V.flen, &V.flen_cap, nfaces + nfaces / 4 + 64));
    J.fsrc = V.fsrc; J.flen = V.flen;
    hipLaunchKernelGGL(k_vo_emit, dim3(vo_blocks(n, VO_THREADS)), dim3(VO_THREADS), 0, st, J);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  }
  for (int k = 0; k < 8; ++k) counts8[k] = (long)w[k];
  V.nfaces = nfaces; V.rcut = rcut;
  V.seq = h->substep_seq; V.moved = h->grains_moved; V.walls = h->walls_moved;
  V.valid = true;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_voronoi_grains(lbmdem_handle* h, double* area, double* perimeter, double* phi, double* R2, int* faces, int* walls,
                                   int* nverts, int* flags) try {
  CHECK_H(h);
  RC_TRY(voronoi_ready(h, "lbmdem_download_voronoi_grains"));
  const size_t n = (size_t)h->n;
  const auto& V = h->vo;
  double* const d[4] = {area, perimeter, phi, R2};
  int* const g[4] = {faces, walls, nverts, flags};
  for (int k = 0; k < 4; ++k) {
    if (d[k]) HIP_TRY(hipMemcpyAsync(d[k], V.dbl + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (g[k]) HIP_TRY(hipMemcpyAsync(g[k], V.ints + k * n, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_voronoi_grains_device(lbmdem_handle* h, const double** area, const double** perimeter, const double** phi, const double** R2,
                                 const int** faces, const int** walls, const int** nverts, const int** flags) try {
  CHECK_H(h);
  RC_TRY(voronoi_ready(h, "lbmdem_voronoi_grains_device"));
  const size_t n = (size_t)h->n;
  const auto& V = h->vo;
  const double** const d[4] = {area, perimeter, phi, R2};
  const int** const g[4] = {faces, walls, nverts, flags};
  for (int k = 0; k < 4; ++k) {
    if (d[k]) *d[k] = V.dbl + k * n;
    if (g[k]) *g[k] = V.ints + k * n;
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_voronoi_faces(lbmdem_handle* h, int* foff, int* fsrc, double* flen, long cap, long* count) try {
  CHECK_H(h);
  if (!count || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(voronoi_ready(h, "lbmdem_download_voronoi_faces"));
  const auto& V = h->vo;
  const long total = V.nfaces;
  *count = total;
  if (cap == 0 && !foff) return LBMDEM_OK;   // (how many there are)
  if (cap > 0 && cap < total)
    return fail(LBMDEM_EINVAL, "lbmdem_download_voronoi_faces: there are %ld faces, the buffers hold %ld", total, cap);
  const size_t n = (size_t)h->n;
  if (foff) HIP_TRY(hipMemcpyAsync(foff, V.ints + 5 * n + 1, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, h->stream));
  if (cap > 0 && total > 0) {
    if (fsrc) HIP_TRY(hipMemcpyAsync(fsrc, V.fsrc, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
    if (flen) HIP_TRY(hipMemcpyAsync(flen, V.flen, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_voronoi(lbmdem_handle* h, const char* dir, int nfile, double rcut) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_voronoi_compute"));
  const size_t n = (size_t)h->n;
  long scounts[8], counts[8];
  RC_TRY(lbmdem_structure_compute(h, rcut, 1, 1.0, (long)INT_MAX, scounts));
  RC_TRY(lbmdem_voronoi_compute(h, counts));
  std::vector<double> d(3 * n);
  std::vector<int> g(4 * n);
  RC_TRY(lbmdem_download_voronoi_grains(h, d.data(), d.data() + n, d.data() + 2 * n, nullptr, g.data(), g.data() + n, g.data() + 2 * n,
                                        g.data() + 3 * n));
  const lbmdem_config& c = h->cfg;
  return lbmdem_write_voronoi_files(dir, nfile, (int)n, d.data(), d.data() + n, d.data() + 2 * n, g.data(), g.data() + n,
                                    g.data() + 2 * n, g.data() + 3 * n, rcut, counts, h->nbsteps * c.dt, c.Mdx - c.Mgx, c.Mhy - c.Mby);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_voronoi_output(lbmdem_handle* h, int on, double rcut) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) {
    RC_TRY(whole_handle(h, "lbmdem_set_voronoi_output"));
    if (!(rcut > 0) || !vo_finite(rcut)) return fail(LBMDEM_EINVAL, "lbmdem_set_voronoi_output: rcut must be finite and > 0 (%le)", rcut);
    h->voronoi_rcut = rcut;
  }
  h->voronoi_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
