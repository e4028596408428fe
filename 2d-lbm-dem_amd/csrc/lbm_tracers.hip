// lbm_tracers.hip -- fluid tracers (lbmdem_tracer_set, lbmdem_tracer_advance, lbmdem_tracer_download, lbmdem_tracer_device,
// lbmdem_tracer_sample, lbmdem_tracer_stats, lbmdem_write_tracers, lbmdem_write_tracers_files, lbmdem_set_tracer_output;
// include/lbmdem_hip.h): massless particles carried by the composite velocity of fluid and grains, one midpoint step per fluid
// step, on the device. The reference has no such routine: the contract is the arithmetic the header spells out, every
// expression associated as written there.
//
//   k_tracer_advance  one lane per tracer, in place. Two stages; a stage reads the owners of the four nodes of the tracer's cell
//                     (the two that differ in y are neighbours along the contiguous axis of obst[x][y] and of
//                     f[x][y / 16][q][y % 16]), then per node the nine populations of a fluid node or the five kinematics of a
//                     grain's (node_vel, lbm_device.h: the flow fields' formulas). Scattered 8-byte loads and nothing else: the
//                     kernel lives on the number of wavefronts in flight, 256 lanes per workgroup, no LDS, no atomics. Gated: an
//                     advance queued behind a launch of k_dem_chain that gave up does nothing, and the replay makes it again.
//   k_tracer_sample   the same gather at the present positions: U, V and the nearest node's owner per tracer.
// The advance only reads the step's state and writes the tracers' own buffer: nothing a later step reads changes. With no
// tracers set nothing is allocated or launched. Double-precision library only: the entry points that take a handle refuse in
// the float build; the host-only file writer exists in both.
// Front end, as every export's: whole_handle(), SP_REFUSE() and reader_obst() (lbmdem_handle.h), MemPool (lbm_mem.h) for the
// buffers kept on the handle, OutFile (lbm_outfile.h) for the file.
#include "lbm_device.h"
#include "lbm_outfile.h"

namespace {

#ifndef LBMDEM_SINGLE_PRECISION
// (TRACER_MAX, lbmdem_handle.h: positions, 2 doubles, and the sample's scratch, 3 doubles, of a set stay under 1 GiB together)
constexpr int TR_THREADS = 256;

struct TracerJob {
  const real* f;
  const int* obst;   // device layout [x][sy]
  LatticeView L;     // (the whole lattice: gx0 == 0, nxl == lx)
  Kin K;
  double* xy;        // [n][2]
  double* uvo;       // [n][3] (the sample)
  long n;
};

// clamp(v) of the header: a NaN goes to 0 and never reaches an index
__device__ __forceinline__ double tracer_clamp(double v, int last) {
  return !(v >= 0.) ? 0. : (v > (double)last ? (double)last : v);
}

// (U, V) at the point (px, py) of [0, lx - 1] x [0, ly - 1]: bilinear in the composite velocity of the cell's four nodes
__device__ __forceinline__ void tracer_vel(const TracerJob& J, double px, double py, double& U, double& V) {
  const LatticeView& L = J.L;
  int i = (int)px, j = (int)py;
  i = i > L.lx - 2 ? L.lx - 2 : i;
  j = j > L.ly - 2 ? L.ly - 2 : j;
  const double a = px - i, b = py - j;
  // the map first: four owners, two 8-byte neighbourhoods; f only where a node is fluid
  const long at = (long)i * L.sy + j;
  const int o00 = J.obst[at], o01 = J.obst[at + 1], o10 = J.obst[at + L.sy], o11 = J.obst[at + L.sy + 1];
  real f[9];
  const NodeVel n00 = node_vel(J.f, o00, L, J.K, i, j, f);
  const NodeVel n10 = node_vel(J.f, o10, L, J.K, i + 1, j, f);
  const NodeVel n01 = node_vel(J.f, o01, L, J.K, i, j + 1, f);
  const NodeVel n11 = node_vel(J.f, o11, L, J.K, i + 1, j + 1, f);
  const double w00 = (1. - a) * (1. - b), w10 = a * (1. - b), w01 = (1. - a) * b, w11 = a * b;
  U = (((w00 * n00.ux) + (w10 * n10.ux)) + (w01 * n01.ux)) + (w11 * n11.ux);
  V = (((w00 * n00.uy) + (w10 * n10.uy)) + (w01 * n01.uy)) + (w11 * n11.uy);
}

__global__ __launch_bounds__(TR_THREADS) void k_tracer_advance(const TracerJob J) {
  LBMDEM_GATE(J.L.gate);
  const long k = (long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (k >= J.n) return;
  const int xl = J.L.lx - 1, yl = J.L.ly - 1;
  double2* slot = reinterpret_cast<double2*>(J.xy) + k;
  const double2 p = *slot;
  // (the identity on what lbmdem_tracer_set accepts and an advance leaves; it keeps a position written through
  // lbmdem_tracer_device away from the indices as well)
  const double px = tracer_clamp(p.x, xl), py = tracer_clamp(p.y, yl);
  double U0, V0, U1, V1;
  tracer_vel(J, px, py, U0, V0);
  const double qx = tracer_clamp(px + 0.5 * U0, xl), qy = tracer_clamp(py + 0.5 * V0, yl);
  tracer_vel(J, qx, qy, U1, V1);
  *slot = double2{tracer_clamp(px + U1, xl), tracer_clamp(py + V1, yl)};
}

__global__ __launch_bounds__(TR_THREADS) void k_tracer_sample(const TracerJob J) {
  const long k = (long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (k >= J.n) return;
  const int xl = J.L.lx - 1, yl = J.L.ly - 1;
  const double2 p = reinterpret_cast<const double2*>(J.xy)[k];
  const double px = tracer_clamp(p.x, xl), py = tracer_clamp(p.y, yl);
  double U, V;
  tracer_vel(J, px, py, U, V);
  const int nx = (int)(px + 0.5), ny = (int)(py + 0.5);   // (<= lx - 1, ly - 1: px + 0.5 <= lx - 0.5)
  J.uvo[3 * k] = U;
  J.uvo[3 * k + 1] = V;
  J.uvo[3 * k + 2] = (double)J.obst[(long)nx * J.L.sy + ny];
}

TracerJob tracer_job(const lbmdem_handle* h, const int* obst) {
  TracerJob J{};
  J.f = h->f[h->fcur];
  J.obst = obst;
  J.L = h->L;
  J.K = h->kin[h->kcur];
  J.xy = h->tracers.xy;
  J.uvo = h->tracers.uvo;
  J.n = h->tracers.n;
  return J;
}

// U, V and the owner at the present positions into the handle's scratch, on the handle's stream
int tracer_sample_launch(lbmdem_handle* h) {
  TracerState& T = h->tracers;
  HIP_TRY(h->mem.grow(&T.uvo, &T.uvo_cap, 3 * T.n));
  TracerJob J = tracer_job(h, reader_obst(h));
  J.L.gate = nullptr;
  hipLaunchKernelGGL(k_tracer_sample, dim3((unsigned)((T.n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}

// the tracers gone and their buffers given back now, not when the handle ends
void tracer_free(lbmdem_handle* h) {
  h->mem.release(h->tracers.xy);
  h->mem.release(h->tracers.uvo);
  h->tracers = TracerState{};
}
#endif   // !LBMDEM_SINGLE_PRECISION

inline unsigned be_float(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return __builtin_bswap32(u);
}

// tracers%.6i.vtk: legacy binary POLYDATA, one vertex per tracer at the coordinates of the frames' mesh
int tracer_write_file(const char* dir, int nfile, int lx, long n, const double* xy, const double* uvo) {
  const float pas = (float)(1. / lx);   // (lbmdem_vtk_put_mesh's)
  const size_t N = (size_t)n;
  std::vector<unsigned> points(3 * N), cells(2 * N), vec(3 * N), owner(N);
  for (size_t k = 0; k < N; ++k) {
    points[3 * k] = be_float((float)xy[2 * k] * pas);
    points[3 * k + 1] = be_float((float)xy[2 * k + 1] * pas);
    points[3 * k + 2] = be_float(0.f);
    cells[2 * k] = __builtin_bswap32(1u);
    cells[2 * k + 1] = __builtin_bswap32((unsigned)k);
    vec[3 * k] = be_float((float)uvo[3 * k]);
    vec[3 * k + 1] = be_float((float)uvo[3 * k + 1]);
    vec[3 * k + 2] = be_float(0.f);
    owner[k] = be_float((float)uvo[3 * k + 2]);
  }
  OutFile F;
  RC_TRY(F.open("w+", dir, "tracers%.6i.vtk", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# vtk DataFile Version 2.0\nlbmdem fluid tracers\nBINARY\nDATASET POLYDATA\n");
  fprintf(fp, "POINTS %ld float\n", n);
  bool short_write = fwrite(points.data(), 4, 3 * N, fp) != 3 * N;
  fprintf(fp, "VERTICES %ld %ld\n", n, 2 * n);
  short_write |= fwrite(cells.data(), 4, 2 * N, fp) != 2 * N;
  fprintf(fp, "POINT_DATA %ld\nVECTORS tracer_velocity_lb float\n", n);
  short_write |= fwrite(vec.data(), 4, 3 * N, fp) != 3 * N;
  fprintf(fp, "SCALARS tracer_owner float\nLOOKUP_TABLE default\n");
  short_write |= fwrite(owner.data(), 4, N, fp) != N;
  return F.close(short_write);
}

}  // namespace

int lbmdem_tracer_launch(lbmdem_handle* h, const int* obst, bool hook) {
#ifdef LBMDEM_SINGLE_PRECISION
  (void)h; (void)obst; (void)hook;
  return fail(LBMDEM_EINVAL, "tracing the fluid is not available in the single-precision build of the library");
#else
  TracerState& T = h->tracers;
  if (T.n <= 0) return LBMDEM_OK;
  const TracerJob J = tracer_job(h, obst);
  hipLaunchKernelGGL(k_tracer_advance, dim3((unsigned)((T.n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  T.advances++;
  if (hook) T.hook++;
  return LBMDEM_OK;
#endif
}

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_write_tracers_files(const char* dir, int nfile, int lx, long n, const double* xy, const double* uvo) try {
  if (n < 0 || lx < 2) return fail(LBMDEM_EINVAL, "lbmdem_write_tracers_files: %ld tracers on a lattice of %d rows", n, lx);
  if (n > 0 && (!xy || !uvo)) return fail(LBMDEM_EINVAL, "null buffer");
  return tracer_write_file(dir, nfile, lx, n, xy, uvo);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_tracer_set(lbmdem_handle* h, long, const double*, int) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_tracer_advance(lbmdem_handle* h) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_tracer_download(lbmdem_handle* h, double*, long, long*) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_tracer_device(lbmdem_handle* h, void**) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_tracer_sample(lbmdem_handle* h, double*, long, long*) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_tracer_stats(lbmdem_handle* h, long*) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_write_tracers(lbmdem_handle* h, const char*, int) { SP_REFUSE(h, "tracing the fluid"); }
int lbmdem_set_tracer_output(lbmdem_handle* h, int) { SP_REFUSE(h, "tracing the fluid"); }
#else

int lbmdem_tracer_set(lbmdem_handle* h, long n, const double* xy, int automatic) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_tracer_set"));
  const LatticeView& L = h->L;
  if (n < 0 || n > TRACER_MAX) return fail(LBMDEM_EINVAL, "lbmdem_tracer_set: 0 to %ld tracers (%ld asked for)", TRACER_MAX, n);
  if (n > 0 && !xy) return fail(LBMDEM_EINVAL, "null buffer");
  if (n > 0 && (L.lx < 2 || L.ly < 2)) return fail(LBMDEM_EINVAL, "lbmdem_tracer_set: the lattice is %d x %d", L.lx, L.ly);
  for (long k = 0; k < n; ++k) {   // (a NaN fails both comparisons of its axis)
    const double px = xy[2 * k], py = xy[2 * k + 1];
    if (!(px >= 0. && px <= (double)(L.lx - 1)) || !(py >= 0. && py <= (double)(L.ly - 1)))
      return fail(LBMDEM_EINVAL, "lbmdem_tracer_set: tracer %ld = (%.17g, %.17g) is not inside [0, %d] x [0, %d]", k, px, py,
                  L.lx - 1, L.ly - 1);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));   // (an advance of the earlier set may be in flight)
  tracer_free(h);
  if (n == 0) return LBMDEM_OK;
  TracerState T{};
  if (h->mem.dev(&T.xy, 2 * (size_t)n) != hipSuccess)
    return fail(LBMDEM_ENOMEM, "lbmdem_tracer_set: device allocation of %zu bytes failed", 2 * sizeof(double) * (size_t)n);
  if (hipMemcpy(T.xy, xy, 2 * sizeof(double) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    h->mem.release(T.xy);
    return fail(LBMDEM_EHIP, "lbmdem_tracer_set: copying the positions to the device failed");
  }
  T.n = n;
  T.automatic = automatic != 0;
  h->tracers = T;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_tracer_advance(lbmdem_handle* h) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_tracer_advance"));
  return lbmdem_tracer_launch(h, reader_obst(h), false);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_tracer_download(lbmdem_handle* h, double* xy, long cap, long* count) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_tracer_download"));
  if (!count || cap < 0 || (cap > 0 && !xy)) return fail(LBMDEM_EINVAL, "null buffer");
  const TracerState& T = h->tracers;
  *count = T.n;
  if (cap == 0) return LBMDEM_OK;   // (how many there are)
  if (cap < T.n) return fail(LBMDEM_EINVAL, "lbmdem_tracer_download: there are %ld tracers, the buffer holds %ld", T.n, cap);
  if (T.n > 0) HIP_TRY(hipMemcpyAsync(xy, T.xy, 2 * sizeof(double) * (size_t)T.n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_tracer_device(lbmdem_handle* h, void** xy) try {
  CHECK_H(h);
  RC_TRY(whole_handle(h, "lbmdem_tracer_device"));
  if (!xy) return fail(LBMDEM_EINVAL, "null argument");
  *xy = h->tracers.xy;   // (null while no tracers are set)
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_tracer_sample(lbmdem_handle* h, double* out3, long cap, long* count) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_tracer_sample"));
  if (!count || cap < 0 || (cap > 0 && !out3)) return fail(LBMDEM_EINVAL, "null buffer");
  TracerState& T = h->tracers;
  *count = T.n;
  if (cap == 0) return LBMDEM_OK;
  if (cap < T.n) return fail(LBMDEM_EINVAL, "lbmdem_tracer_sample: there are %ld tracers, the buffer holds %ld", T.n, cap);
  if (T.n > 0) {
    RC_TRY(tracer_sample_launch(h));
    HIP_TRY(hipMemcpyAsync(out3, T.uvo, 3 * sizeof(double) * (size_t)T.n, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_tracer_stats(lbmdem_handle* h, long* counts3) try {
  CHECK_H(h);   // (settles: the counts are those of the advances that took place)
  RC_TRY(whole_handle(h, "lbmdem_tracer_stats"));
  if (!counts3) return fail(LBMDEM_EINVAL, "null argument");
  counts3[0] = h->tracers.n; counts3[1] = h->tracers.advances; counts3[2] = h->tracers.hook;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_tracers(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  RC_TRY(whole_handle(h, "lbmdem_write_tracers"));
  if (!dir) return fail(LBMDEM_EINVAL, "null directory");
  TracerState& T = h->tracers;
  std::vector<double> xy(2 * (size_t)T.n), uvo(3 * (size_t)T.n);
  if (T.n > 0) {
    RC_TRY(tracer_sample_launch(h));
    HIP_TRY(hipMemcpyAsync(xy.data(), T.xy, sizeof(double) * xy.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(uvo.data(), T.uvo, sizeof(double) * uvo.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // (the file shows a position written through lbmdem_tracer_device as the kernels read it)
    for (size_t k = 0; k < xy.size(); ++k) {
      const double last = (double)((k & 1 ? h->L.ly : h->L.lx) - 1);
      xy[k] = !(xy[k] >= 0.) ? 0. : (xy[k] > last ? last : xy[k]);
    }
  }
  return tracer_write_file(dir, nfile, h->L.lx, T.n, xy.data(), uvo.data());
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_tracer_output(lbmdem_handle* h, int on) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) RC_TRY(whole_handle(h, "lbmdem_set_tracer_output"));
  h->tracer_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
