// lbmdem_output.hip -- the reference's file outputs over the C ABI: write_vtk (main.c:237-338 + visit_writer's binary
// rectilinear path), write_DEM (main.c:340-438: DEM%06d.dat, stats.data), write_forces (main.c:440-478), the per-grain
// diagnostics table they print, the merged-strip forms of the VTK writer, and the frames, tables and checkpoints written in the
// background (lbmdem_set_async_output, lbmdem_set_async_dem, lbmdem_set_async_checkpoint: snapshot kernels, copy stream, writer
// thread).

#include "lbmdem_handle.h"

#include <chrono>
#include <errno.h>
#include <system_error>

#pragma GCC visibility push(default)
extern "C" {
int lbmdem_download_vtk_fields(lbmdem_handle* h, float* grain_pressure, float* grain_velocity,
                               float* grain_acceleration, float* fluid_pressure, float* fluid_velocity) {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!grain_pressure || !grain_velocity || !grain_acceleration || !fluid_pressure || !fluid_velocity)
    return fail(LBMDEM_EINVAL, "null buffer");
  const LatticeView& L = h->L;
  const size_t cnt = (size_t)(L.xo1 - L.xo0) * L.ly;
  MemPool scratch;
  float* tmp = nullptr;
  HIP_TRY(scratch.dev(&tmp, cnt * 11));
  float *d_gp = tmp, *d_gv = tmp + cnt, *d_ga = tmp + 4 * cnt, *d_fp = tmp + 7 * cnt, *d_fv = tmp + 8 * cnt;
  const Kin& K = h->kin[h->kcur];
  launch_vtk_fields(h->f[h->fcur], reader_obst(h), L, h->gp, K.v1, K.v2, K.a1, K.a2, h->cfg.phys.rho_moy, d_gp, d_gv, d_ga,
                    d_fp, d_fv, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(grain_pressure, d_gp, sizeof(float) * cnt, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(grain_velocity, d_gv, sizeof(float) * cnt * 3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(grain_acceleration, d_ga, sizeof(float) * cnt * 3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fluid_pressure, d_fp, sizeof(float) * cnt, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fluid_velocity, d_fv, sizeof(float) * cnt * 3, hipMemcpyDeviceToHost));
  return LBMDEM_OK;
}

// One legacy-VTK file: binary, big-endian float32, RECTILINEAR_GRID with one point-data variable --
// the byte layout the reference obtains from write_rectilinear_mesh(..., useBinary = 1, ...)
// (main.c:326-328): header, DIMENSIONS, X/Y/Z_COORDINATES, CELL_DATA, POINT_DATA, one SCALARS
// (+ LOOKUP_TABLE default) or VECTORS block, no separators after binary blocks.
static const char* const VTK_NAMES[5] = {"grain_pressure", "grain_velocity", "grain_acceleration", "fluid_pressure", "fluid_velocity"};
static const int VTK_DIMS[5] = {1, 3, 3, 1, 3};

static void put_be(FILE* fp, const float* v, size_t n) {
  std::vector<unsigned char> buf(n * 4);
  for (size_t k = 0; k < n; ++k) {
    unsigned char b[4];
    memcpy(b, &v[k], 4);
    buf[4 * k] = b[3]; buf[4 * k + 1] = b[2]; buf[4 * k + 2] = b[1]; buf[4 * k + 3] = b[0];
  }
  fwrite(buf.data(), 1, buf.size(), fp);
}

// header, mesh and the CELL_DATA / POINT_DATA lines: everything in front of the first variable (also lbm_flow.hip's file)
void lbmdem_vtk_put_mesh(FILE* fp, int nx, int ny) {
  fprintf(fp, "# vtk DataFile Version 2.0\nWritten using VisIt writer\nBINARY\n");
  fprintf(fp, "DATASET RECTILINEAR_GRID\nDIMENSIONS %d %d 1\n", nx, ny);
  // coordinates: i * (float)(1/nx) on BOTH axes, z = 0 (main.c:255-258)
  const float pas = 1. / nx;
  std::vector<float> xs(nx), ys(ny);
  for (int i = 0; i < nx; ++i) xs[i] = i * pas;
  for (int i = 0; i < ny; ++i) ys[i] = i * pas;
  const float z = 0.f;
  fprintf(fp, "X_COORDINATES %d float\n", nx); put_be(fp, xs.data(), nx);
  fprintf(fp, "Y_COORDINATES %d float\n", ny); put_be(fp, ys.data(), ny);
  fprintf(fp, "Z_COORDINATES 1 float\n"); put_be(fp, &z, 1);
  fprintf(fp, "CELL_DATA %d\nPOINT_DATA %d\n", (nx - 1) * (ny - 1), nx * ny);
}

// everything in front of the variable's payload
static void put_vtk_head(FILE* fp, int nx, int ny, const char* name, int dim) {
  lbmdem_vtk_put_mesh(fp, nx, ny);
  if (dim == 1) fprintf(fp, "SCALARS %s float\nLOOKUP_TABLE default\n", name);
  else fprintf(fp, "VECTORS %s float\n", name);
}

int lbmdem_write_vtk_file(const char* path, int nx, int ny, const char* name, int dim, const float* data) {
  FILE* fp = fopen(path, "w+");
  if (!fp) return fail(LBMDEM_EINVAL, "cannot open '%s' for writing", path);
  put_vtk_head(fp, nx, ny, name, dim);
  put_be(fp, data, (size_t)nx * ny * dim);
  fclose(fp);
  return LBMDEM_OK;
}

int lbmdem_write_vtk(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  const LatticeView& L = h->L;
  if (L.xo0 != 0 || L.xo1 != L.lx || L.gx0 != 0)
    return fail(LBMDEM_EINVAL, "lbmdem_write_vtk needs the whole lattice on this handle; gather strips with "
                               "lbmdem_download_vtk_fields");
  const size_t cnt = (size_t)L.lx * L.ly;
  std::vector<float> f11(11 * cnt);
  float* f = f11.data();
  RC_TRY(lbmdem_download_vtk_fields(h, f, f + cnt, f + 4 * cnt, f + 7 * cnt, f + 8 * cnt));
  return lbmdem_write_vtk_fields(dir, nfile, L.lx, L.ly, f);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

int lbmdem_set_diagnostics(lbmdem_handle* h, int always) {
  SP_UNAVAILABLE("the write_DEM diagnostics table");
  CHECK_H(h);   // (always-diagnose keeps the multi-sub-step kernel out: unconfirmed launches are settled with the old setting)
  h->diag_always = always != 0;
  return LBMDEM_OK;
}

// 30 columns per grain in the reference's struct order (main.c:182-197):
// x1 x2 x3 v1 v2 v3 a1 a2 a3 r m mw It p s f1 f2 ifm fm fr ifr M11 M12 M21 M22 ice slip rw z zz
int lbmdem_download_grain_table(lbmdem_handle* h, double* t) try {
  SP_UNAVAILABLE("the write_DEM diagnostics table");
  CHECK_H(h);
  if (!t) return fail(LBMDEM_EINVAL, "null buffer");
  if (!h->diag_valid) return fail(LBMDEM_EINVAL, "no contact diagnostics for the last sub-step (lbmdem_set_diagnostics, or "
                                                 "the sub-step that reaches a multiple of 4000)");
  const int n = h->n;
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::vector<double> kin(9 * (size_t)n), rr(n), mm(n), it(n), gp(n), dg(9 * (size_t)n), ex(4 * (size_t)n);
  HIP_TRY(hipMemcpy(ex.data(), h->dx.fr, sizeof(double) * 4 * n, hipMemcpyDeviceToHost));  // fr, ice, slip, rw
  HIP_TRY(hipMemcpy(kin.data(), h->kin[h->kcur].x1, sizeof(double) * 9 * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rr.data(), h->r, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(mm.data(), h->m, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(it.data(), h->It, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gp.data(), h->gp, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dg.data(), h->diag, sizeof(double) * 9 * n, hipMemcpyDeviceToHost));
  const int* zi = reinterpret_cast<const int*>(dg.data() + 8 * (size_t)n);
  const lbmdem_config& c = h->cfg;
  for (int i = 0; i < n; ++i) {
    double* o = t + (size_t)i * 30;
    for (int k = 0; k < 9; ++k) o[k] = kin[(size_t)k * n + i];
    o[9] = rr[i]; o[10] = mm[i]; o[11] = 0.0; o[12] = it[i];
    o[13] = gp[i]; o[14] = dg[i]; o[15] = dg[(size_t)n + i]; o[16] = dg[2 * (size_t)n + i];
    o[17] = dg[3 * (size_t)n + i];
    const int z = zi[i], zz = zi[n + i];
    o[18] = (z == 0) ? 0. : o[17] / z;  // fm, main.c:409-412
    o[19] = ex[i];                      // fr
    // ifr, main.c:388-390
    o[20] = fabs(((o[10] * c.phys.G + o[16]) * (c.dt * o[4] + c.dt2 * o[7] / 2.)) + (o[15] * (c.dt * o[3] + c.dt2 * o[6] / 2.)));
    o[21] = dg[4 * (size_t)n + i]; o[22] = dg[5 * (size_t)n + i]; o[23] = dg[6 * (size_t)n + i]; o[24] = dg[7 * (size_t)n + i];
    o[25] = ex[(size_t)n + i]; o[26] = ex[2 * (size_t)n + i]; o[27] = ex[3 * (size_t)n + i];  // ice, slip, rw
    o[28] = z; o[29] = zz;
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

// ---- the table as text: ONE formatter and ONE pair search for the synchronous writers and the writer thread ---------------------
// `rows`: LBMDEM_DEM_ROW_DOUBLES per grain -- r x1 x2 x3 v1 v2 v3 a1 a2 a3 fhf1 fhf2 fhf3 p s ESE fr ifr ice slip rw fm M11
// M12 M21 M22 z zz: the columns of main.c:413-420 after the index, then zz. On failure the text goes to `msg`, not to the
// thread's error text (the writer thread reports through its job).
static_assert(LBMDEM_DEM_ROW_DOUBLES == DEM_ROW, "the rows of k_dem_frame are the rows of the ABI");

static int close_checked(FILE* fp, const char* path, char* msg, size_t msglen) {
  const bool bad = ferror(fp) != 0;
  const int err = errno;
  if (fclose(fp) != 0 || bad) {
    snprintf(msg, msglen, "writing '%s' failed: %s", path, strerror(bad ? err : errno));
    return LBMDEM_EINVAL;
  }
  return LBMDEM_OK;
}

// DEM%06d.dat (28 tab-separated columns per grain) and one line appended to stats.data, main.c:413-434
static int write_dem_text(const char* dir, int nfile, int n, const double* rows, const double* stats22, char* msg, size_t msglen) {
  char path[4200];
  snprintf(path, sizeof path, "%s/DEM%.6i.dat", (dir && *dir) ? dir : ".", nfile);
  FILE* fp = fopen(path, "w");
  if (!fp) { snprintf(msg, msglen, "cannot open '%s' for writing", path); return LBMDEM_EINVAL; }
  for (int i = 0; i < n; i++) {
    const double* o = rows + (size_t)i * LBMDEM_DEM_ROW_DOUBLES;
    fprintf(fp,
            "%i\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%le\t%i\n",
            i, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11], o[12], o[13], o[14], o[15], o[16],
            o[17], o[18], o[19], o[20], o[21], o[22], o[23], o[24], o[25], (int)o[26]);
  }
  int rc = close_checked(fp, path, msg, msglen);
  if (rc != LBMDEM_OK) return rc;
  snprintf(path, sizeof path, "%s/stats.data", (dir && *dir) ? dir : ".");
  fp = fopen(path, "a");
  if (!fp) { snprintf(msg, msglen, "cannot open '%s' for appending", path); return LBMDEM_EINVAL; }
  const double* t = stats22;
  fprintf(fp, "%le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le %le\n", t[0], t[1], t[2],
          t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11], t[12], t[13], t[14], t[15], t[16], t[17], t[18], t[19], t[20],
          t[21]);
  return close_checked(fp, path, msg, msglen);
}

// DEM%06d.ps, main.c:440-478. The four columns it needs from a table of `stride` doubles per grain: centre, radius, fm.
struct MapCols { const double* base; size_t stride; int x1, x2, r, fm; };

static int write_forces_text(const char* dir, int nfile, int n, MapCols T, int lx, int ly, char* msg, size_t msglen) try {
  auto X1 = [&](int i) { return T.base[(size_t)i * T.stride + T.x1]; };
  auto X2 = [&](int i) { return T.base[(size_t)i * T.stride + T.x2]; };
  auto R = [&](int i) { return T.base[(size_t)i * T.stride + T.r]; };
  char path[4200];
  snprintf(path, sizeof path, "%s/DEM%.6i.ps", (dir && *dir) ? dir : ".", nfile);
  FILE* fp = fopen(path, "w");
  if (!fp) { snprintf(msg, msglen, "cannot open '%s' for writing", path); return LBMDEM_EINVAL; }
  lbmdem_ps_head(fp, n, T.base + T.x1, T.base + T.x2, T.base + T.r, T.base + T.fm, T.stride, lx, ly);
  // overlapping pairs, dn < -1e-10 (main.c:462-466), found on a uniform grid of cell size 2 r_max: any pair
  // with dn < 0 has its centres closer than that, i.e. in adjacent cells
  double xmin = X1(0), xmax = X1(0), ymin = X2(0), ymax = X2(0), rmax = R(0);
  for (int i = 1; i < n; i++) {
    if (X1(i) < xmin) xmin = X1(i);
    if (X1(i) > xmax) xmax = X1(i);
    if (X2(i) < ymin) ymin = X2(i);
    if (X2(i) > ymax) ymax = X2(i);
    if (R(i) > rmax) rmax = R(i);
  }
  const double cs = 2 * rmax > 0 ? 2 * rmax : 1.0;
  long ncx = (long)((xmax - xmin) / cs) + 1, ncy = (long)((ymax - ymin) / cs) + 1;
  while (ncx * ncy > 4L * n + 64) {  // far-flung grains: coarsen (still correct, cells only get larger)
    if (ncx >= ncy) ncx = (ncx + 1) / 2; else ncy = (ncy + 1) / 2;
  }
  const double csx = (xmax - xmin) / ncx > cs ? (xmax - xmin) / ncx * (1 + 1e-12) : cs;
  const double csy = (ymax - ymin) / ncy > cs ? (ymax - ymin) / ncy * (1 + 1e-12) : cs;
  auto cell = [&](double v, double lo, double c, long nc) {
    long k = (long)((v - lo) / c);
    return k < 0 ? 0 : (k >= nc ? nc - 1 : k);
  };
  std::vector<int> start((size_t)(ncx * ncy) + 1, 0), order(n);
  for (int i = 0; i < n; i++) start[(size_t)(cell(X2(i), ymin, csy, ncy) * ncx + cell(X1(i), xmin, csx, ncx)) + 1]++;
  for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; i++) order[(size_t)fill[(size_t)(cell(X2(i), ymin, csy, ncy) * ncx + cell(X1(i), xmin, csx, ncx))]++] = i;
  }
  std::vector<int> js;
  for (int i = 0; i < n; i++) {
    js.clear();
    const long cx = cell(X1(i), xmin, csx, ncx), cy = cell(X2(i), ymin, csy, ncy);
    for (long yy = cy - 1; yy <= cy + 1; ++yy) {
      if (yy < 0 || yy >= ncy) continue;
      for (long xx = cx - 1; xx <= cx + 1; ++xx) {
        if (xx < 0 || xx >= ncx) continue;
        for (int k = start[(size_t)(yy * ncx + xx)]; k < start[(size_t)(yy * ncx + xx) + 1]; ++k) {
          const int j = order[(size_t)k];
          if (j == i) continue;
          const double dn = (sqrt((X1(i) - X1(j)) * (X1(i) - X1(j)) + (X2(i) - X2(j)) * (X2(i) - X2(j)))) - R(i) - R(j);
          if (dn < -1e-10) js.push_back(j);
        }
      }
    }
    for (size_t a = 1; a < js.size(); ++a) {  // ascending j: the reference's inner loop order
      const int v = js[a];
      size_t b = a;
      while (b > 0 && js[b - 1] > v) { js[b] = js[b - 1]; --b; }
      js[b] = v;
    }
    for (int j : js) {
      fprintf(fp, "%le setlinewidth \n 0.0 setgray \n", 1.);
      fprintf(fp, "1 setlinecap \n newpath \n");
      fprintf(fp, "%le %le moveto \n %le %le lineto\n", X1(i) * 10000, X2(i) * 10000, X1(j) * 10000, X2(j) * 10000);
      fprintf(fp, "stroke \n");
    }
  }
  return close_checked(fp, path, msg, msglen);
} catch (const std::bad_alloc&) {
  snprintf(msg, msglen, "host memory allocation failed");
  return LBMDEM_ENOMEM;
}

static int write_dem_rows_files(const char* dir, int nfile, int n, const double* rows, const double* stats22, int with_forces,
                                int lx, int ly, char* msg, size_t msglen) {
  const int rc = write_dem_text(dir, nfile, n, rows, stats22, msg, msglen);
  if (rc != LBMDEM_OK || !with_forces) return rc;
  return write_forces_text(dir, nfile, n, MapCols{rows, LBMDEM_DEM_ROW_DOUBLES, 1, 2, 0, 21}, lx, ly, msg, msglen);
}

int lbmdem_write_dem_rows(const char* dir, int nfile, int n, const double* rows, const double* stats22, int with_forces, int lx,
                          int ly) {
  if (n < 1 || !rows || !stats22) return fail(LBMDEM_EINVAL, "bad lbmdem_write_dem_rows arguments");
  char msg[4400];
  const int rc = write_dem_rows_files(dir, nfile, n, rows, stats22, with_forces, lx, ly, msg, sizeof msg);
  return rc == LBMDEM_OK ? rc : fail(rc, "%s", msg);
}

// write_DEM, main.c:340-438: DEM%06d.dat and one line appended to stats.data, from the table brought to the host.
// energies8 (may be NULL): KE, PE, SE, IFR, WF, INCE, TSLIP, TRW.
int lbmdem_write_dem(lbmdem_handle* h, const char* dir, int nfile, double* energies8) try {
  SP_UNAVAILABLE("write_DEM");
  CHECK_H(h);
  const int n = h->n;
  std::vector<double> t(30 * (size_t)n), hf(3 * (size_t)n), rows(LBMDEM_DEM_ROW_DOUBLES * (size_t)n);
  int rc = lbmdem_download_grain_table(h, t.data());
  if (rc != LBMDEM_OK) return rc;
  rc = lbmdem_download_fhf(h, hf.data());
  if (rc != LBMDEM_OK) return rc;
  const lbmdem_config& c = h->cfg;
  const lbmdem_physics& p = c.phys;
  auto G = [&](int i, int col) { return t[(size_t)i * 30 + col]; };
  double xfront = G(0, 0) + G(0, 9), height = G(0, 1) + G(0, 9), xgrainmax = G(0, 0);
  double energie_x = 0., energie_y = 0., energie_teta = 0., energy_p = 0., SE = 0., IFR = 0., zmean = 0;
  double WF = 0., INCE = 0., TSLIP = 0., TRW = 0.;
  double N[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    const double x1 = G(i, 0), x2 = G(i, 1), v1 = G(i, 3), v2 = G(i, 4), v3 = G(i, 5), r = G(i, 9), m = G(i, 10),
                 It = G(i, 12), pp = G(i, 13), ss = G(i, 14);
    const int z = (int)G(i, 28), zz = (int)G(i, 29);
    zmean += z;
    if (z >= 0 && z <= 5) N[z] += 1;
    energie_x += 0.5 * m * v1 * v1;
    energie_y += 0.5 * m * v2 * v2;
    energie_teta += 0.5 * It * v3 * v3;
    energy_p += m * p.G * x2;
    SE += 0.5 * (((pp * pp) / p.kg) + ((ss * ss) / p.kt));
    WF += G(i, 19);
    IFR += G(i, 20);
    TSLIP += G(i, 26);
    TRW += G(i, 27);
    INCE += G(i, 25);
    const double ESE = 0.5 * (((pp * pp) / p.kg) + ((ss * ss) / p.kt));
    if (x1 + r > xgrainmax) xgrainmax = x1 + r;
    if (x2 + r > height) height = x2 + r;
    if (zz > 0 && x1 + r >= xfront) xfront = x1 + r;
    const double row[LBMDEM_DEM_ROW_DOUBLES] = {
        r, x1, x2, G(i, 2), v1, v2, v3, G(i, 6), G(i, 7), G(i, 8), hf[3 * (size_t)i], hf[3 * (size_t)i + 1],
        hf[3 * (size_t)i + 2], pp, ss, ESE, G(i, 19), G(i, 20), G(i, 25), G(i, 26), G(i, 27), G(i, 18), G(i, 21),
        G(i, 22), G(i, 23), G(i, 24), (double)z, (double)zz};
    memcpy(&rows[(size_t)i * LBMDEM_DEM_ROW_DOUBLES], row, sizeof row);
  }
  const double energie_cin = energie_x + energie_y + energie_teta;
  zmean = zmean / n;
  const double stats22[22] = {h->nbsteps * c.dt - p.dtt, xfront, xgrainmax, height, zmean, energie_x, energie_y, energie_teta,
                              energie_cin, N[0] / n, N[1] / n, N[2] / n, N[3] / n, N[4] / n, N[5] / n, energy_p, SE, WF, IFR,
                              INCE, TSLIP, TRW};
  char msg[4400];
  rc = write_dem_text(dir, nfile, n, rows.data(), stats22, msg, sizeof msg);
  if (rc != LBMDEM_OK) return fail(rc, "%s", msg);
  if (energies8) {
    energies8[0] = energie_cin; energies8[1] = energy_p; energies8[2] = SE; energies8[3] = IFR;
    energies8[4] = WF; energies8[5] = INCE; energies8[6] = TSLIP; energies8[7] = TRW;
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

int lbmdem_write_forces(lbmdem_handle* h, const char* dir, int nfile) try {
  SP_UNAVAILABLE("write_forces");
  CHECK_H(h);
  const int n = h->n;
  std::vector<double> t(30 * (size_t)n);
  int rc = lbmdem_download_grain_table(h, t.data());
  if (rc != LBMDEM_OK) return rc;
  char msg[4400];
  rc = write_forces_text(dir, nfile, n, MapCols{t.data(), 30, 0, 1, 9, 18}, h->cfg.lx, h->cfg.ly, msg, sizeof msg);
  return rc == LBMDEM_OK ? rc : fail(rc, "%s", msg);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

// a strip's five fields (block11: the layout of lbmdem_download_vtk_fields for nx columns, back to back) into the
// lattice-sized arrays, columns [x0, x0 + nx)
int lbmdem_vtk_place_block(float* fields11, int lx, int ly, int x0, int nx, const float* block11) {
  const size_t part = (size_t)nx * ly, cnt = (size_t)lx * ly;
  const float* lp[5] = {block11, block11 + part, block11 + 4 * part, block11 + 7 * part, block11 + 8 * part};
  float* fp[5] = {fields11, fields11 + cnt, fields11 + 4 * cnt, fields11 + 7 * cnt, fields11 + 8 * cnt};
  for (int k = 0; k < 5; ++k)
    for (int y = 0; y < ly; ++y)
      memcpy(fp[k] + ((size_t)y * lx + x0) * VTK_DIMS[k], lp[k] + (size_t)y * nx * VTK_DIMS[k], sizeof(float) * nx * VTK_DIMS[k]);
  return LBMDEM_OK;
}

// write_vtk of a strip decomposition (main.c:237-338): every rank drops its owned columns into zero-initialised
// lattice-sized arrays (fields11 = grain_pressure[cnt], grain_velocity[3 cnt], grain_acceleration[3 cnt],
// fluid_pressure[cnt], fluid_velocity[3 cnt], cnt = lx * ly, each [ly][lx]); the caller merges the ranks' arrays
// (disjoint columns) and one rank writes the five files with lbmdem_write_vtk_fields.
int lbmdem_vtk_place_owned(lbmdem_handle* h, float* fields11) try {
  CHECK_H(h);
  if (!fields11) return fail(LBMDEM_EINVAL, "null buffer");
  const LatticeView& L = h->L;
  const int nx = L.xo1 - L.xo0, x0 = L.gx0 + L.xo0;
  const size_t part = (size_t)nx * L.ly;
  std::vector<float> loc(11 * part);
  float* lp[5] = {loc.data(), loc.data() + part, loc.data() + 4 * part, loc.data() + 7 * part, loc.data() + 8 * part};
  int rc = lbmdem_download_vtk_fields(h, lp[0], lp[1], lp[2], lp[3], lp[4]);
  if (rc != LBMDEM_OK) return rc;
  lbmdem_vtk_place_block(fields11, L.lx, L.ly, x0, nx, loc.data());
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}


int lbmdem_write_vtk_fields(const char* dir, int nfile, int lx, int ly, const float* fields11) {
  if (!fields11 || lx < 2 || ly < 2) return fail(LBMDEM_EINVAL, "bad lbmdem_write_vtk_fields arguments");
  const size_t cnt = (size_t)lx * ly;
  const float* data[5] = {fields11, fields11 + cnt, fields11 + 4 * cnt, fields11 + 7 * cnt, fields11 + 8 * cnt};
  for (int k = 0; k < 5; ++k) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s_%.6i.vtk", (dir && *dir) ? dir : ".", VTK_NAMES[k], nfile);  // main.c:241-249
    RC_TRY(lbmdem_write_vtk_file(path, lx, ly, VTK_NAMES[k], VTK_DIMS[k], data[k]));
  }
  return LBMDEM_OK;
}

// ---- frames, tables and checkpoints in the background ------------------------------------------------------------------
// The image: the five payloads as the files hold them, back to back (k_vtk_frame, lbm_frame.hip).

// the five files from an image; on failure the text goes to `msg`, not to the thread's error text (the writer thread
// reports through its job)
static int write_image_files(const char* dir, int nfile, int nx, int ny, const void* image, char* msg, size_t msglen) try {
  const size_t cnt = (size_t)nx * ny;
  const unsigned char* at = static_cast<const unsigned char*>(image);
  for (int k = 0; k < 5; ++k) {
    char path[4200];
    snprintf(path, sizeof path, "%s/%s_%.6i.vtk", (dir && *dir) ? dir : ".", VTK_NAMES[k], nfile);  // main.c:241-249
    FILE* fp = fopen(path, "w+");
    if (!fp) { snprintf(msg, msglen, "cannot open '%s' for writing", path); return LBMDEM_EINVAL; }
    put_vtk_head(fp, nx, ny, VTK_NAMES[k], VTK_DIMS[k]);
    const size_t bytes = cnt * 4 * VTK_DIMS[k];
    const bool short_write = fwrite(at, 1, bytes, fp) != bytes;
    const int err = errno;
    if (fclose(fp) != 0 || short_write) {
      snprintf(msg, msglen, "writing '%s' failed: %s", path, strerror(short_write ? err : errno));
      return LBMDEM_EINVAL;
    }
    at += bytes;
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  snprintf(msg, msglen, "host memory allocation failed");
  return LBMDEM_ENOMEM;
}

static inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the writer thread: job by job in the order they were queued -- wait for the copy, write the files, free the slot
static void async_writer(AsyncOut* a) {
  (void)hipSetDevice(a->device);
  for (;;) {
    AsyncJob job;
    {
      std::unique_lock<std::mutex> lk(a->mu);
      a->cv_job.wait(lk, [&] { return a->quit || !a->jobs.empty(); });
      if (a->jobs.empty()) return;
      job = a->jobs.front();
      a->jobs.pop_front();
    }
    AsyncSlot& S = a->lane[job.kind].slot[job.slot];
    char msg[sizeof a->err_msg];
    int code = LBMDEM_EHIP;
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipEventSynchronize(S.copied);
    const double ms_copy = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    if (e != hipSuccess && job.kind == ASYNC_CKPT) {
      snprintf(msg, sizeof msg, "checkpoint '%.4000s': the copy to host memory failed: %s", S.path, hipGetErrorString(e));
    } else if (e != hipSuccess) {
      snprintf(msg, sizeof msg, "%s %d: the copy to host memory failed: %s", ASYNC_KIND_NAMES[job.kind], S.nfile, hipGetErrorString(e));
    } else switch (job.kind) {
      case ASYNC_FRAME:
        code = write_image_files(S.path, S.nfile, a->lx, a->ly, S.pinned, msg, sizeof msg);
        break;
      case ASYNC_TABLE:
        code = write_dem_rows_files(S.path, S.nfile, a->n, static_cast<const double*>(S.pinned), S.stats22, S.with_forces, a->lx,
                                    a->ly, msg, sizeof msg);
        break;
#ifndef LBMDEM_SINGLE_PRECISION
      case ASYNC_CKPT:
        code = lbmdem_ckpt_write_slot(&S, msg, sizeof msg);   // (from the slot's own layout)
        break;
#endif
    }
    const double ms_io = ms_since(t1);
    {
      std::lock_guard<std::mutex> lk(a->mu);
      AsyncCounters& C = a->lane[job.kind].c;
      C.ms_copy_wait += ms_copy;
      C.ms_io += ms_io;
      if (code == LBMDEM_OK) C.written++;
      else {
        C.failed++;
        if (!a->err_code) { a->err_code = code; a->err_kind = job.kind; memcpy(a->err_msg, msg, sizeof msg); }
      }
      S.busy = false;
      a->pending--;
    }
    a->cv_free.notify_all();
  }
}

// a kind's slots and counters (the table's scratch is its caller's)
static void lane_free(AsyncOut* a, int kind) {
  for (AsyncSlot& S : a->lane[kind].slot) {
    a->mem.release(S.staging);
    a->mem.release(S.pinned);
    if (S.snapped) (void)hipEventDestroy(S.snapped);
    if (S.copied) (void)hipEventDestroy(S.copied);
    S.staging = S.pinned = nullptr;
    S.snapped = S.copied = nullptr;
  }
  a->lane[kind].slots = 0;
  a->lane[kind].c = AsyncCounters{};
}

static void dem_scratch_free(AsyncOut* a) {
  a->mem.release(a->dem_scratch);
  a->mem.release(a->dem_stats_host);
  a->dem_scratch = a->dem_stats_host = nullptr;
}

static void async_free(AsyncOut* a) {
  for (int kind = 0; kind < ASYNC_KINDS; ++kind) lane_free(a, kind);
  dem_scratch_free(a);
  if (a->copy_stream) (void)hipStreamDestroy(a->copy_stream);
  delete a;
}

// everything queued is on disk: the writer sleeps, no slot is in use
static void async_wait_idle(AsyncOut* a, std::unique_lock<std::mutex>& lk) {
  a->cv_free.wait(lk, [&] { return a->pending == 0; });
}

void lbmdem_async_wait_idle(lbmdem_handle* h) {
  if (!h->aout) return;
  std::unique_lock<std::mutex> lk(h->aout->mu);
  async_wait_idle(h->aout, lk);
}

void lbmdem_async_release(lbmdem_handle* h) {
  AsyncOut* a = h->aout;
  if (!a) return;
  {
    std::unique_lock<std::mutex> lk(a->mu);
    async_wait_idle(a, lk);
    a->quit = true;
  }
  a->cv_job.notify_all();
  if (a->writer.joinable()) a->writer.join();
  async_free(a);
  h->aout = nullptr;
}

int lbmdem_async_report(lbmdem_handle* h) {
  AsyncOut* a = h->aout;
  if (!a) return LBMDEM_OK;
  char msg[sizeof a->err_msg];
  int code, kind;
  {
    std::lock_guard<std::mutex> lk(a->mu);
    code = a->err_code;
    if (code == LBMDEM_OK) return LBMDEM_OK;
    memcpy(msg, a->err_msg, sizeof msg);
    kind = a->err_kind;
    a->err_code = LBMDEM_OK;
  }
  return fail(code, "background %s writer: %s", ASYNC_KIND_NAMES[kind], msg);
}

// What the three kinds share -- the AsyncOut, its copy stream and its writer thread -- made when the first of them is switched on
static int async_ensure(lbmdem_handle* h, const char* who) {
  if (h->aout) return LBMDEM_OK;
  AsyncOut* a = new (std::nothrow) AsyncOut;
  if (!a) return fail(LBMDEM_ENOMEM, "host memory allocation failed");
  a->lx = h->L.lx; a->ly = h->L.ly; a->n = h->n; a->device = h->cfg.device;
  const hipError_t e = hipStreamCreateWithFlags(&a->copy_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    async_free(a);
    return fail(LBMDEM_ENOMEM, "%s: the copy stream cannot be had: %s", who, hipGetErrorString(e));
  }
  try {
    a->writer = std::thread(async_writer, a);
  } catch (const std::system_error&) {
    async_free(a);
    return fail(LBMDEM_ENOMEM, "%s: the writer thread cannot be started", who);
  }
  h->aout = a;
  return LBMDEM_OK;
}

// The last kind went off: the writer thread and the copy stream go with it
static void async_release_if_unused(lbmdem_handle* h) {
  for (int kind = 0; kind < ASYNC_KINDS; ++kind) if (lane_on(h, kind)) return;
  lbmdem_async_release(h);
}

// A kind's number of slots changes, or their size (`who`: the setter, `noun`: what a slot holds). The request is carried out
// first: everything queued is written, the old slots are freed, the new ones made, `bytes` of device staging and of pinned host
// memory each; a failure of the writer that nobody has been told about is taken out beforehand and is what the call then returns.
static int lane_resize(lbmdem_handle* h, int kind, int slots, size_t bytes, const char* who, const char* noun) {
  if ((h->aout ? h->aout->lane[kind].slots : 0) == slots && (slots == 0 || h->aout->lane[kind].bytes == bytes)) return LBMDEM_OK;
  int old_code = LBMDEM_OK, old_kind = ASYNC_FRAME;
  char old_msg[sizeof AsyncOut::err_msg];
  if (AsyncOut* a = h->aout) {
    {
      std::unique_lock<std::mutex> lk(a->mu);
      async_wait_idle(a, lk);
      old_code = a->err_code;
      old_kind = a->err_kind;
      if (old_code != LBMDEM_OK) memcpy(old_msg, a->err_msg, sizeof old_msg);
      a->err_code = LBMDEM_OK;
    }
    lane_free(a, kind);
    if (kind == ASYNC_TABLE) dem_scratch_free(a);
  }
  if (slots > 0) {
    RC_TRY(async_ensure(h, who));
    AsyncOut* a = h->aout;
    hipError_t e = hipSuccess;
    if (kind == ASYNC_TABLE) {
      e = a->mem.dev(&a->dem_scratch, DEM_STATS_CHAINS * (size_t)a->n + 22);
      if (e == hipSuccess) e = a->mem.pinned(&a->dem_stats_host, 22);
    }
    for (int s = 0; s < slots && e == hipSuccess; ++s) {
      AsyncSlot& S = a->lane[kind].slot[s];
      e = a->mem.dev(&S.staging, bytes);
      if (e == hipSuccess) e = a->mem.pinned(&S.pinned, bytes);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&S.snapped, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&S.copied, hipEventDisableTiming | hipEventBlockingSync);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      lane_free(a, kind);
      if (kind == ASYNC_TABLE) dem_scratch_free(a);
      async_release_if_unused(h);
      return fail(LBMDEM_ENOMEM, "%s: %d %s slots of %zu bytes (device staging + pinned host memory each) cannot be had: %s", who,
                  slots, noun, bytes, hipGetErrorString(e));
    }
    a->lane[kind].slots = slots;
    a->lane[kind].bytes = bytes;
  }
  async_release_if_unused(h);
  if (old_code != LBMDEM_OK) return fail(old_code, "background %s writer: %s", ASYNC_KIND_NAMES[old_kind], old_msg);
  return LBMDEM_OK;
}

// A free slot of the kind, marked busy. Back-pressure: with none free the caller waits for the writer, a job is never dropped.
static int lane_acquire(AsyncOut* a, int kind) {
  AsyncLane& Ln = a->lane[kind];
  std::unique_lock<std::mutex> lk(a->mu);
  auto free_slot = [&] { for (int k = 0; k < Ln.slots; ++k) if (!Ln.slot[k].busy) return k; return -1; };
  int s = free_slot();
  if (s < 0) {
    const auto t0 = std::chrono::steady_clock::now();
    Ln.c.slot_waits++;
    a->cv_free.wait(lk, [&] { return (s = free_slot()) >= 0; });
    Ln.c.ms_slot_wait += ms_since(t0);
  }
  Ln.slot[s].busy = true;
  return s;
}

// Behind what the handle's stream holds so far -- the slot's snapshot -- the copy stream takes the staging to the pinned buffer
static hipError_t slot_copy_behind(lbmdem_handle* h, AsyncOut* a, AsyncSlot& S, size_t bytes) {
  hipError_t e = hipEventRecord(S.snapped, h->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(a->copy_stream, S.snapped, 0);
  if (e == hipSuccess) e = hipMemcpyAsync(S.pinned, S.staging, bytes, hipMemcpyDeviceToHost, a->copy_stream);
  if (e == hipSuccess) e = hipEventRecord(S.copied, a->copy_stream);
  return e;
}

// A job that could not be launched: its slot is free again
static void lane_abandon(AsyncOut* a, AsyncSlot& S) {
  (void)hipStreamSynchronize(a->copy_stream);   // (whatever part was queued no longer touches the slot)
  { std::lock_guard<std::mutex> lk(a->mu); S.busy = false; }
  a->cv_free.notify_all();
}

// ... and one that was: the writer's from here (ms_last: AsyncCounters)
static void lane_commit(AsyncOut* a, int kind, int s, double ms_last) {
  {
    std::lock_guard<std::mutex> lk(a->mu);
    a->jobs.push_back(AsyncJob{kind, s});
    a->pending++;
    a->lane[kind].c.queued++;
    a->lane[kind].c.ms_last += ms_last;
  }
  a->cv_job.notify_one();
}

static int output_stats_of(lbmdem_handle* h, int kind, long* counts4, double* ms4) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  AsyncCounters C;
  if (AsyncOut* a = h->aout) {
    std::lock_guard<std::mutex> lk(a->mu);
    C = a->lane[kind].c;
  }
  const long c[4] = {C.queued, C.written, C.failed, C.slot_waits};
  const double m[4] = {C.ms_slot_wait, C.ms_copy_wait, C.ms_io, C.ms_last};
  for (int k = 0; k < 4; ++k) { if (counts4) counts4[k] = c[k]; if (ms4) ms4[k] = m[k]; }
  return LBMDEM_OK;
}

// whole_handle()'s `instead`: what the owner of a strip or of distributed grains calls for a frame, a table, a checkpoint
#define FRAME_THERE "use lbmdem_comm_write_vtk there"
#define TABLE_THERE "there rank 0 writes the tables with lbmdem_write_dem"
#define CKPT_THERE "there every rank saves its own file with lbmdem_checkpoint_save"

static void launch_frame(lbmdem_handle* h, void* image_dev) {
  const Kin& K = h->kin[h->kcur];
  launch_vtk_frame(h->f[h->fcur], reader_obst(h), h->L, h->gp, K.v1, K.v2, K.a1, K.a2, h->cfg.phys.rho_moy, image_dev, h->stream);
}

size_t lbmdem_vtk_image_bytes(int lx, int ly) { return (lx > 0 && ly > 0) ? (size_t)44 * lx * ly : 0; }

int lbmdem_write_vtk_image(const char* dir, int nfile, int lx, int ly, const void* image_be) {
  if (!image_be || lx < 2 || ly < 2) return fail(LBMDEM_EINVAL, "bad lbmdem_write_vtk_image arguments");
  char msg[4400];
  const int rc = write_image_files(dir, nfile, lx, ly, image_be, msg, sizeof msg);
  return rc == LBMDEM_OK ? rc : fail(rc, "%s", msg);
}

int lbmdem_download_vtk_image(lbmdem_handle* h, void* image_be) {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!image_be) return fail(LBMDEM_EINVAL, "null buffer");
  RC_TRY(whole_handle(h, "lbmdem_download_vtk_image", FRAME_THERE));
  const size_t bytes = lbmdem_vtk_image_bytes(h->L.lx, h->L.ly);
  MemPool scratch;
  void* tmp = nullptr;
  HIP_TRY(scratch.dev(&tmp, bytes));
  launch_frame(h, tmp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(image_be, tmp, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
}

// ---- frames ----------------------------------------------------------------------------------------------------------------

int lbmdem_set_async_output(lbmdem_handle* h, int frames) {
  CHECK_H(h);
  if (frames < 0 || frames > LBMDEM_ASYNC_MAX_FRAMES)
    return fail(LBMDEM_EINVAL, "lbmdem_set_async_output: frames must be 0..%d, not %d", LBMDEM_ASYNC_MAX_FRAMES, frames);
  if (frames > 0) RC_TRY(whole_handle(h, "lbmdem_set_async_output", FRAME_THERE));
  return lane_resize(h, ASYNC_FRAME, frames, lbmdem_vtk_image_bytes(h->L.lx, h->L.ly), "lbmdem_set_async_output", "frame");
}

int lbmdem_write_vtk_async(lbmdem_handle* h, const char* dir, int nfile) {
  CHECK_H(h);   // (a launch of k_dem_chain that gave up is undone and replayed here: nothing unconfirmed lies ahead of the snapshot)
  AsyncOut* a = h->aout;
  if (!async_frames_on(h)) return fail(LBMDEM_EINVAL, "lbmdem_write_vtk_async: async output is off (lbmdem_set_async_output)");
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_write_vtk_async", FRAME_THERE));
  RC_TRY(lbmdem_async_report(h));   // an earlier frame's failure: this call queues nothing
  const char* d = (dir && *dir) ? dir : ".";
  if (strlen(d) >= sizeof AsyncSlot::path) return fail(LBMDEM_EINVAL, "lbmdem_write_vtk_async: directory name too long");
  const int s = lane_acquire(a, ASYNC_FRAME);
  AsyncSlot& S = a->lane[ASYNC_FRAME].slot[s];
  strcpy(S.path, d);
  S.nfile = nfile;
  launch_frame(h, S.staging);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = slot_copy_behind(h, a, S, a->lane[ASYNC_FRAME].bytes);
  if (e != hipSuccess) {
    lane_abandon(a, S);
    HIP_TRY(e);
  }
  lane_commit(a, ASYNC_FRAME, s, 0.);
  return LBMDEM_OK;
}

int lbmdem_output_drain(lbmdem_handle* h) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  AsyncOut* a = h->aout;
  if (!a) return LBMDEM_OK;
  {
    std::unique_lock<std::mutex> lk(a->mu);
    if (a->pending != 0) {
      const auto t0 = std::chrono::steady_clock::now();
      async_wait_idle(a, lk);
      if (a->lane[ASYNC_FRAME].slots) a->lane[ASYNC_FRAME].c.ms_last += ms_since(t0);   // (lbmdem_output_stats is all 0 while frames are off)
    }
  }
  return lbmdem_async_report(h);
}

int lbmdem_output_stats(lbmdem_handle* h, long* counts4, double* ms4) { return output_stats_of(h, ASYNC_FRAME, counts4, ms4); }

// ---- tables ----------------------------------------------------------------------------------------------------------------

#ifndef LBMDEM_SINGLE_PRECISION
static DemTableView dem_table_view(const lbmdem_handle* h) {
  const lbmdem_config& c = h->cfg;
  return DemTableView{h->n, h->kin[h->kcur], h->r, h->m, h->It, h->gp, h->diag, h->dx.fr, h->dx.ice, h->dx.slip, h->dx.rw,
                      h->fhf, c.phys.G, c.dt, c.dt2, c.phys.kg, c.phys.kt};
}
#endif

#define CHECK_TABLE(h)                                                                                                           \
  do {                                                                                                                           \
    if (!(h)->diag_valid || !(h)->dx_ready)                                                                                      \
      return fail(LBMDEM_EINVAL, "no contact diagnostics for the last sub-step (lbmdem_set_diagnostics, or the sub-step that "  \
                                 "reaches a multiple of 4000)");                                                                 \
  } while (0)

int lbmdem_dem_stats(lbmdem_handle* h, double* stats22) {
  SP_UNAVAILABLE("write_DEM");
#ifndef LBMDEM_SINGLE_PRECISION
  CHECK_H(h);
  if (!stats22) return fail(LBMDEM_EINVAL, "null buffer");
  CHECK_TABLE(h);
  const size_t n = (size_t)h->n;
  MemPool own;             // (the scratch of the background writer, where there is one: it is idle between two events)
  double* scratch = async_dem_on(h) ? h->aout->dem_scratch : nullptr;
  if (!scratch) HIP_TRY(own.dev(&scratch, DEM_STATS_CHAINS * n + 22));
  const DemTableView T = dem_table_view(h);
  launch_dem_frame(T, nullptr, scratch, h->stream);
  launch_dem_stats(T, scratch, scratch + DEM_STATS_CHAINS * n, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(stats22, scratch + DEM_STATS_CHAINS * n, sizeof(double) * 22, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  stats22[0] = h->nbsteps * h->cfg.dt - h->cfg.phys.dtt;   // main.c:428
  return LBMDEM_OK;
#endif
}

int lbmdem_set_async_dem(lbmdem_handle* h, int slots) {
  SP_UNAVAILABLE("write_DEM");
#ifndef LBMDEM_SINGLE_PRECISION
  CHECK_H(h);
  if (slots < 0 || slots > LBMDEM_ASYNC_MAX_DEM)
    return fail(LBMDEM_EINVAL, "lbmdem_set_async_dem: slots must be 0..%d, not %d", LBMDEM_ASYNC_MAX_DEM, slots);
  if (slots > 0) RC_TRY(whole_handle(h, "lbmdem_set_async_dem", TABLE_THERE));
  return lane_resize(h, ASYNC_TABLE, slots, sizeof(double) * LBMDEM_DEM_ROW_DOUBLES * (size_t)h->n, "lbmdem_set_async_dem", "table");
#endif
}

int lbmdem_write_dem_async(lbmdem_handle* h, const char* dir, int nfile, int with_forces, double* energies8) {
  SP_UNAVAILABLE("write_DEM");
#ifndef LBMDEM_SINGLE_PRECISION
  CHECK_H(h);   // (a launch of k_dem_chain that gave up is undone and replayed here: the table is the confirmed one)
  if (!async_dem_on(h)) return fail(LBMDEM_EINVAL, "lbmdem_write_dem_async: tables in the background are off (lbmdem_set_async_dem)");
  AsyncOut* a = h->aout;
  RC_TRY(whole_handle(h, "lbmdem_write_dem_async", TABLE_THERE));
  CHECK_TABLE(h);
  RC_TRY(lbmdem_async_report(h));   // an earlier job's failure: this call queues nothing
  const char* d = (dir && *dir) ? dir : ".";
  if (strlen(d) >= sizeof AsyncSlot::path) return fail(LBMDEM_EINVAL, "lbmdem_write_dem_async: directory name too long");
  const int s = lane_acquire(a, ASYNC_TABLE);
  AsyncSlot& S = a->lane[ASYNC_TABLE].slot[s];
  strcpy(S.path, d);
  S.nfile = nfile;
  S.with_forces = with_forces != 0;
  double* stats_dev = a->dem_scratch + DEM_STATS_CHAINS * (size_t)a->n;
  const DemTableView T = dem_table_view(h);
  launch_dem_frame(T, static_cast<double*>(S.staging), a->dem_scratch, h->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = slot_copy_behind(h, a, S, a->lane[ASYNC_TABLE].bytes);   // the rows are complete: their copy may start under k_dem_stats
  if (e == hipSuccess) { launch_dem_stats(T, a->dem_scratch, stats_dev, h->stream); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpyAsync(a->dem_stats_host, stats_dev, sizeof(double) * 22, hipMemcpyDeviceToHost, h->stream);
  const auto t0 = std::chrono::steady_clock::now();
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // the 22 numbers: the only wait on the step stream
  const double ms_stats = ms_since(t0);
  if (e != hipSuccess) {
    lane_abandon(a, S);
    HIP_TRY(e);
  }
  memcpy(S.stats22, a->dem_stats_host, sizeof S.stats22);
  S.stats22[0] = h->nbsteps * h->cfg.dt - h->cfg.phys.dtt;   // main.c:428
  if (energies8) {
    const double* t = S.stats22;
    energies8[0] = t[8]; energies8[1] = t[15]; energies8[2] = t[16]; energies8[3] = t[18];
    energies8[4] = t[17]; energies8[5] = t[19]; energies8[6] = t[20]; energies8[7] = t[21];
  }
  lane_commit(a, ASYNC_TABLE, s, ms_stats);
  return LBMDEM_OK;
#endif
}

int lbmdem_output_stats_dem(lbmdem_handle* h, long* counts4, double* ms4) { return output_stats_of(h, ASYNC_TABLE, counts4, ms4); }

// ---- checkpoints -----------------------------------------------------------------------------------------------------------

int lbmdem_set_async_checkpoint(lbmdem_handle* h, int slots) {
  SP_UNAVAILABLE("checkpointing");
#ifndef LBMDEM_SINGLE_PRECISION
  CHECK_H(h);
  if (slots < 0 || slots > LBMDEM_ASYNC_MAX_CKPT)
    return fail(LBMDEM_EINVAL, "lbmdem_set_async_checkpoint: slots must be 0..%d, not %d", LBMDEM_ASYNC_MAX_CKPT, slots);
  if (slots > 0) RC_TRY(whole_handle(h, "lbmdem_set_async_checkpoint", CKPT_THERE));
  // the file of the handle as it stands: with the optional state lbmdem_set_checkpoint_contents selects, where the handle has
  // it now (lbmdem_checkpoint_save_async makes the slots larger when a later checkpoint needs more)
  CkptShot C;
  const CkptLayout Y = lbmdem_ckpt_shot(h, &C);
  return lane_resize(h, ASYNC_CKPT, slots, Y.total, "lbmdem_set_async_checkpoint", "checkpoint");
#endif
}

int lbmdem_checkpoint_save_async(lbmdem_handle* h, const char* path) {
  SP_UNAVAILABLE("checkpointing");
#ifndef LBMDEM_SINGLE_PRECISION
  CHECK_H(h);   // (a launch of k_dem_chain that gave up is undone and replayed here: the checkpoint is the confirmed state's)
  if (!async_ckpt_on(h)) return fail(LBMDEM_EINVAL, "lbmdem_checkpoint_save_async: checkpoints in the background are off (lbmdem_set_async_checkpoint)");
  AsyncOut* a = h->aout;
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_checkpoint_save_async", CKPT_THERE));
  if (!path || !*path) return fail(LBMDEM_EINVAL, "null path");
  if (strlen(path) >= sizeof AsyncSlot::path) return fail(LBMDEM_EINVAL, "lbmdem_checkpoint_save_async: path too long");
  if (h->obst_pending) return fail(LBMDEM_EINVAL, "checkpoint between obst_construction and collide_stream");
  RC_TRY(lbmdem_async_report(h));   // an earlier job's failure: this call queues nothing
  // the layout is the job's: optional state may have appeared or gone since the last checkpoint was queued. The host's side of
  // the header is taken as of now: the run goes on behind this call
  CkptShot C;
  const CkptLayout Y = lbmdem_ckpt_shot(h, &C);
  if (Y.total > a->lane[ASYNC_CKPT].bytes) {   // the state has outgrown the slots: as many, larger ones (drains the lane first)
    const int slots = a->lane[ASYNC_CKPT].slots;
    AsyncCounters kept;
    { std::unique_lock<std::mutex> lk(a->mu); async_wait_idle(a, lk); kept = a->lane[ASYNC_CKPT].c; }
    const int rc = lane_resize(h, ASYNC_CKPT, slots, Y.total, "lbmdem_checkpoint_save_async", "checkpoint");
    a = h->aout;   // (LBMDEM_ENOMEM: the lane is as lane_resize leaves it, off, and `a` may be gone with it)
    if (async_ckpt_on(h)) { std::lock_guard<std::mutex> lk(a->mu); a->lane[ASYNC_CKPT].c = kept; }   // the counters are the feature's, not the slots'
    RC_TRY(rc);
  }
  const int s = lane_acquire(a, ASYNC_CKPT);
  const auto t_hold = std::chrono::steady_clock::now();
  AsyncSlot& S = a->lane[ASYNC_CKPT].slot[s];
  strcpy(S.path, path);
  S.ckpt_layout = Y;
  S.ckpt_bytes = Y.total;
  S.shot = C;
  if (h->carry_from < h->substep_seq) launch_carry_resolve(h->ct, h->carry_from, h->stream);   // as lbmdem_checkpoint_save
  CkptFrameJob J;
  lbmdem_ckpt_frame_job(h, S.ckpt_layout, static_cast<unsigned char*>(S.staging), &J);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemsetAsync(S.staging, 0, CKPT_WORDS_BYTES, h->stream);   // the digests are sums: from zero
  if (e == hipSuccess) { launch_ckpt_frame(J, h->stream); e = hipGetLastError(); }
  if (e == hipSuccess) e = slot_copy_behind(h, a, S, S.ckpt_bytes);   // the job's bytes, not the lane's capacity
  if (e != hipSuccess) {
    lane_abandon(a, S);
    HIP_TRY(e);
  }
  lane_commit(a, ASYNC_CKPT, s, ms_since(t_hold));
  return LBMDEM_OK;
#endif
}

int lbmdem_output_stats_checkpoint(lbmdem_handle* h, long* counts4, double* ms4) { return output_stats_of(h, ASYNC_CKPT, counts4, ms4); }

}  // extern "C"
#pragma GCC visibility pop
