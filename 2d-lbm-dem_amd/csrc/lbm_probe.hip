// lbm_probe.hip -- device-side probes (lbmdem_probe_*, include/lbmdem_hip.h): the field diagnostics the reference has
// routines for but never calls -- write_densities' basal pressure profile (main.c:522-541), velocity_profile
// (main.c:1647-1676), pressures (main.c:1681-1694), xgrainmax / height of write_DEM (main.c:400-405) -- recorded on the
// handle's stream right after forces_fluid of a fluid step, one short launch per sample, into a ring of records on the
// device. The host takes no part until lbmdem_probe_read. With the probes off (the default) nothing here is reached.
// Double-precision library only: the float build refuses lbmdem_probe_enable.
// Unlike the exports' front ends (whole_handle(), SP_REFUSE(), lbmdem_handle.h) it refuses a strip in words of its own and
// only where it is switched on; its buffers are released by name (lbmdem_probe_disable) and it writes no file.
#include "lbm_device.h"
#include "lbmdem_handle.h"

namespace {

constexpr size_t PROBE_MAX_BYTES = (size_t)1 << 30;   // capacity x record size the ring may take

#ifndef LBMDEM_SINGLE_PRECISION
constexpr int PROBE_BLOCK = 256;
constexpr int PROBE_MAX_BLOCKS = 64;   // 16 cover a row of 4096 nodes; the grains' maxima stride over the rest
// One sample. Record layout (doubles): off[0] step, time, clock | off[1] pressure_row[lx] | off[2] the velocity profile's
// row index | off[3] velocity_row[lx] | off[4] point_pressure[npoints] | off[5] xgrainmax, height; off < 0: field off.
struct ProbeJob {
  const real* f;
  const int* obst;
  LatticeView L;
  const real *x1, *x2, *v2, *r;
  int n;
  real rho_moy;
  int prow, npoints;
  const int* points;     // [npoints][2]
  double* ring;          // [capacity][rec], zero where no record has been written (the maxima rely on it)
  long rec;
  int capacity;
  long off[6];
  // {records written, samples dropped} twice: a launch reads pair `parity` and leaves the pair for the next launch in the
  // other one -- every workgroup of a launch sees the same count without a grid-wide fence, the launches of a stream being
  // ordered
  long long* ctr;
  int parity;
  double step, time, clock;
};

__global__ __launch_bounds__(PROBE_BLOCK) void k_probe_sample(const ProbeJob J) {
  LBMDEM_GATE(J.L.gate);
  const LatticeView& L = J.L;
  const long long w = J.ctr[2 * J.parity], dropped = J.ctr[2 * J.parity + 1];
  const bool full = w >= J.capacity;
  const int tid = blockIdx.x * PROBE_BLOCK + threadIdx.x, nthreads = gridDim.x * PROBE_BLOCK;
  if (tid == 0) {   // when the ring is full the sample is dropped and counted, never overwritten and never waited for
    J.ctr[2 * (1 - J.parity)] = full ? w : w + 1;
    J.ctr[2 * (1 - J.parity) + 1] = full ? dropped + 1 : dropped;
  }
  if (full) return;
  double* rec = J.ring + w * J.rec;
  if (tid == 0) { rec[J.off[0]] = J.step; rec[J.off[0] + 1] = J.time; rec[J.off[0] + 2] = J.clock; }
  // a fixed y over all x is a strided walk through f[x][y / 16][q][y % 16]: one lane per x, nine 8-byte loads each
  if (J.off[1] >= 0) {   // main.c:524-539, row y = prow
    const int y = J.prow;
    for (int x = tid; x < L.lx; x += nthreads) {
      const long b = fbase_xy(L, x, y);
      real P = 0.;
      for (int i = 0; i < 9; ++i) P += J.f[b + i * F_QSTRIDE(L)];
      P = (1. / 3.) * J.rho_moy * (P - 1.);
      rec[J.off[1] + x] = J.obst[(long)x * L.sy + y] < 0 ? P : 0.0;
    }
  }
  if (J.off[3] >= 0) {   // main.c:1658-1672
    int y = (int)((J.x2[0] - L.Mby) / L.dx);
    y = y < 0 ? 0 : (y > L.ly - 1 ? L.ly - 1 : y);   // (the reference indexes with it as it is)
    if (tid == 0) rec[J.off[2]] = (double)y;
    for (int x = tid; x < L.lx; x += nthreads) {
      const int o = J.obst[(long)x * L.sy + y];
      real u_y1;
      if (o != -1 && o != L.n) u_y1 = J.v2[o] / L.c;
      else {
        const long b = fbase_xy(L, x, y);
        real u_y = 0, d_loc = 0.;
        for (int i = 0; i < 9; ++i) d_loc = d_loc + J.f[b + i * F_QSTRIDE(L)];
        for (int i = 0; i < 9; ++i) u_y = u_y + J.f[b + i * F_QSTRIDE(L)] * EYq(i);
        u_y1 = u_y / d_loc;
      }
      rec[J.off[3] + x] = u_y1;
    }
  }
  if (J.off[4] >= 0) {   // main.c:1685-1691
    for (int k = tid; k < J.npoints; k += nthreads) {
      const int x = J.points[2 * k], y = J.points[2 * k + 1];
      const long b = fbase_xy(L, x, y);
      const real* p = J.f + b;
      const long q = F_QSTRIDE(L);
      const real c_squ = 1. / 3.;
      const real s = (p[0] + p[q] + p[2 * q] + p[3 * q] + p[4 * q] + p[5 * q] + p[6 * q] + p[7 * q] + p[8 * q] - J.rho_moy) * c_squ;
      rec[J.off[4] + k] = J.obst[(long)x * L.sy + y] == -1 ? s : 0.;
    }
  }
  if (J.off[5] >= 0) {   // main.c:400-405: maxima, so order-free and exact
    real mx = 0., my = 0.;
    for (int i = tid; i < J.n; i += nthreads) {
      const real ri = J.r[i], ax = J.x1[i] + ri, ay = J.x2[i] + ri;
      mx = ax > mx ? ax : mx;
      my = ay > my ? ay : my;
    }
    // within the wavefront, then the workgroup, then ONE atomic per workgroup and value on the bit pattern (the order of
    // non-negative doubles is the order of their bits). INVARIANT the atomics rest on: the two slots of a record that has not
    // been written hold +0.0 -- probe_clear (below) is the one place that makes it so, for the whole ring at
    // lbmdem_probe_enable and for the records handed out by lbmdem_probe_read; a dropped or gated sample writes nothing.
    // Values that are not positive (a packing lies at positive coordinates) never reach the atomic: the result is then 0.
    for (int d = 32; d > 0; d >>= 1) {
      const real ox = __shfl_xor(mx, d), oy = __shfl_xor(my, d);
      mx = ox > mx ? ox : mx;
      my = oy > my ? oy : my;
    }
    __shared__ real sx[PROBE_BLOCK / 64], sy[PROBE_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) { sx[threadIdx.x >> 6] = mx; sy[threadIdx.x >> 6] = my; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < PROBE_BLOCK / 64; ++k) { mx = sx[k] > mx ? sx[k] : mx; my = sy[k] > my ? sy[k] : my; }
      unsigned long long* out = reinterpret_cast<unsigned long long*>(rec + J.off[5]);
      if (mx > 0.) atomicMax(out, (unsigned long long)__double_as_longlong(mx));
      if (my > 0.) atomicMax(out + 1, (unsigned long long)__double_as_longlong(my));
    }
  }
}
#endif

// the first `records` records of the ring back to all-zero, on the handle's stream in front of the next sample (k_probe_sample's
// maxima start from the +0.0 this leaves)
hipError_t probe_clear(const ProbeState& P, long records, hipStream_t st) {
  return records > 0 ? hipMemsetAsync(P.ring, 0, sizeof(double) * (size_t)P.rec * (size_t)records, st) : hipSuccess;
}

// the recorder off and its buffers given back now, not when the handle ends
void probe_free(MemPool& mem, ProbeState& P) {
  mem.release(P.ring);
  mem.release(P.ctr);
  mem.release(P.points);
  P = ProbeState{};
}

}  // namespace

// the ring and its counters as `issued` samples since the ring was last emptied leave them: the first `capacity` kept, the
// rest counted as dropped (what the launches themselves have written, unless a launch of k_dem_chain gave up in between).
// Drains the handle's stream and copies from the stack, blocking: for the recovery path and lbmdem_probe_read only, and it
// must not run while launches that read the counters are in flight on ANOTHER stream (samples go to the handle's stream alone).
int lbmdem_probe_sync_counters(lbmdem_handle* h) {
  ProbeState& P = h->probe;
  if (!P.on) return LBMDEM_OK;
  const long long w = P.issued < P.capacity ? P.issued : P.capacity, d = P.issued - w;
  const long long both[4] = {w, d, w, d};
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(P.ctr, both, sizeof both, hipMemcpyHostToDevice));
  return LBMDEM_OK;
}

// behind the force kernels of a fluid step (lbmdem_forces_fluid): `obst` is the map they have just used
int lbmdem_probe_sample(lbmdem_handle* h, const int* obst) {
#ifdef LBMDEM_SINGLE_PRECISION
  (void)obst;
  return fail(LBMDEM_EINVAL, "probes are not available in the single-precision build of the library");
#else
  ProbeState& P = h->probe;
  const bool due = P.seen % P.every == 0;
  P.seen++;
  if (!due) return LBMDEM_OK;
  const Kin& K = h->kin[h->kcur];
  ProbeJob J{};
  J.f = h->f[h->fcur]; J.obst = obst; J.L = h->L;
  J.x1 = K.x1; J.x2 = K.x2; J.v2 = K.v2; J.r = h->r; J.n = h->n;
  J.rho_moy = (real)h->cfg.phys.rho_moy;
  J.prow = P.pressure_row; J.npoints = P.npoints; J.points = P.points;
  J.ring = P.ring; J.rec = P.rec; J.capacity = P.capacity;
  for (int k = 0; k < 6; ++k) J.off[k] = P.off[k];
  J.ctr = P.ctr; J.parity = (int)(P.issued & 1);
  J.step = (double)h->nbsteps; J.time = h->nbsteps * h->cfg.dt; J.clock = h->vib ? h->cfg.phys.t : 0.;
  const int most = h->L.lx > h->n ? h->L.lx : h->n;
  int blocks = (most + PROBE_BLOCK - 1) / PROBE_BLOCK;
  if (blocks > PROBE_MAX_BLOCKS) blocks = PROBE_MAX_BLOCKS;
  hipLaunchKernelGGL(k_probe_sample, dim3(blocks), dim3(PROBE_BLOCK), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  P.issued++;
  return LBMDEM_OK;
#endif
}

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_probe_disable(lbmdem_handle* h) try {
  CHECK_H(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  probe_free(h->mem, h->probe);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_probe_enable(lbmdem_handle* h, const lbmdem_probe_config* pc) try {
  CHECK_H(h);
  SP_UNAVAILABLE("lbmdem_probe_enable");
  if (!pc) return fail(LBMDEM_EINVAL, "null probe configuration");
  const lbmdem_config& c = h->cfg;
  if (c.x_begin > 0 || c.x_end < c.lx || h->dist)
    return fail(LBMDEM_EINVAL, "probes need the whole lattice on one handle (not a strip of a decomposition, not distributed grains)");
  if (pc->every < 1 || pc->capacity < 1) return fail(LBMDEM_EINVAL, "probes: every and capacity must be at least 1");
  if (pc->pressure_row >= c.ly) return fail(LBMDEM_EINVAL, "probes: pressure_row %d is outside the lattice (ly = %d)", pc->pressure_row, c.ly);
  if (pc->npoints < 0 || pc->npoints > LBMDEM_PROBE_MAX_POINTS || (pc->npoints > 0 && !pc->points))
    return fail(LBMDEM_EINVAL, "probes: 0 to %d points", LBMDEM_PROBE_MAX_POINTS);
  for (int k = 0; k < pc->npoints; ++k)
    if (pc->points[2 * k] < 0 || pc->points[2 * k] >= c.lx || pc->points[2 * k + 1] < 0 || pc->points[2 * k + 1] >= c.ly)
      return fail(LBMDEM_EINVAL, "probes: point %d = (%d, %d) is outside the %d x %d lattice", k, pc->points[2 * k], pc->points[2 * k + 1], c.lx, c.ly);
  ProbeState P{};
  P.every = pc->every; P.capacity = pc->capacity; P.pressure_row = pc->pressure_row; P.npoints = pc->npoints;
  long at = 0;
  P.off[0] = at; at += 3;
  P.off[1] = pc->pressure_row >= 0 ? at : -1; if (pc->pressure_row >= 0) at += c.lx;
  P.off[2] = pc->velocity_row ? at : -1;      if (pc->velocity_row) at += 1;
  P.off[3] = pc->velocity_row ? at : -1;      if (pc->velocity_row) at += c.lx;
  P.off[4] = pc->npoints > 0 ? at : -1;       at += pc->npoints;
  P.off[5] = pc->grain_extent ? at : -1;      if (pc->grain_extent) at += 2;
  P.rec = at;
  const size_t bytes = sizeof(double) * (size_t)P.rec * (size_t)P.capacity;
  if (bytes > PROBE_MAX_BYTES)
    return fail(LBMDEM_EINVAL, "probes: %d records of %ld doubles are more than the %zu MiB a ring may take", P.capacity, P.rec, PROBE_MAX_BYTES >> 20);
  HIP_TRY(hipStreamSynchronize(h->stream));
  probe_free(h->mem, h->probe);
  if (h->mem.dev(&P.ring, (size_t)P.rec * (size_t)P.capacity) != hipSuccess || h->mem.dev(&P.ctr, 4) != hipSuccess ||
      (P.npoints > 0 && h->mem.dev(&P.points, 2 * (size_t)P.npoints) != hipSuccess)) {
    probe_free(h->mem, P);
    return fail(LBMDEM_ENOMEM, "probes: device allocation of %zu bytes failed", bytes);
  }
  h->probe = P;
  h->probe.on = true;
  if (probe_clear(P, P.capacity, h->stream) != hipSuccess || hipMemsetAsync(P.ctr, 0, 4 * sizeof(long long), h->stream) != hipSuccess ||
      (P.npoints > 0 && hipMemcpy(P.points, pc->points, 2 * sizeof(int) * P.npoints, hipMemcpyHostToDevice) != hipSuccess)) {
    probe_free(h->mem, h->probe);
    return fail(LBMDEM_EHIP, "probes: initialising the ring failed");
  }
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

long lbmdem_probe_record_doubles(lbmdem_handle* h) try {
  CHECK_H(h);
  if (!h->probe.on) return fail(LBMDEM_EINVAL, "probes are not enabled on this handle");
  return h->probe.rec;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_probe_layout(lbmdem_handle* h, long* offsets6) try {
  CHECK_H(h);
  if (!offsets6 || !h->probe.on) return fail(LBMDEM_EINVAL, "probes are not enabled on this handle");
  for (int k = 0; k < 6; ++k) offsets6[k] = h->probe.off[k];
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_probe_read(lbmdem_handle* h, double* out, long cap_records, long* count, long* dropped) try {
  CHECK_H(h);
  ProbeState& P = h->probe;
  if (!P.on) return fail(LBMDEM_EINVAL, "probes are not enabled on this handle");
  HIP_TRY(hipStreamSynchronize(h->stream));
  long long ctr[2] = {0, 0};
  HIP_TRY(hipMemcpy(ctr, P.ctr + 2 * (P.issued & 1), sizeof ctr, hipMemcpyDeviceToHost));
  if (count) *count = (long)ctr[0];
  if (dropped) *dropped = (long)ctr[1];
  if (!out) return LBMDEM_OK;   // (how many there are; the ring stays as it is)
  if (cap_records < ctr[0]) return fail(LBMDEM_EINVAL, "lbmdem_probe_read: the ring holds %lld records, the buffer %ld", ctr[0], cap_records);
  const size_t bytes = sizeof(double) * (size_t)P.rec * (size_t)ctr[0];
  if (bytes) {
    HIP_TRY(hipMemcpy(out, P.ring, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(probe_clear(P, (long)ctr[0], h->stream));
  }
  P.issued = 0;
  return lbmdem_probe_sync_counters(h);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

}  // extern "C"
#pragma GCC visibility pop
