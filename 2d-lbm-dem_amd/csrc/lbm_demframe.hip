// lbm_demframe.hip -- the table of a write_DEM event taken on the device: the rows of DEM%06d.dat in the file's order
// (k_dem_frame) and the 22 numbers of the stats.data line (k_dem_stats), main.c:340-438. The arithmetic is that of the host
// loops of lbmdem_download_grain_table / lbmdem_write_dem (lbmdem_output.hip), statement for statement, with the same
// association (-ffp-contract=off); only where it runs differs. Double build only: the float library has no write_DEM.

#include "lbm_device.h"

#ifndef LBMDEM_SINGLE_PRECISION

namespace {

constexpr int ROW = DEM_ROW;                   // r x1 x2 x3 v1 v2 v3 a1 a2 a3 fhf1 fhf2 fhf3 p s ESE fr ifr ice slip rw fm M11 M12 M21 M22 z zz
constexpr int NCHAIN = DEM_STATS_CHAINS;      // energie_x energie_y energie_teta energy_p SE WF IFR INCE TSLIP TRW

// ---- k_dem_frame: one lane per grain ---------------------------------------------------------------------------------------
//   in:  the SoA arrays, lane i reads element i of each: every load of a wavefront is one run of 512 bytes;
//   LDS: the workgroup's rows, [grain][28] with a pitch of 29 doubles (a lane writes its own row: the odd pitch spreads the
//        8-byte writes of a half-wavefront over all 64 banks);
//   out: the rows of FRAME_G consecutive grains are ONE run of FRAME_G * 224 bytes of the image: lanes walk it element by
//        element, 8-byte stores, 512 bytes per wavefront and instruction -- no lane strides by a row;
//        the addends of the ten serial sums of the stats line, SoA [10][n] (k_dem_stats adds them up in grain order).
// rows == nullptr: the addends only (lbmdem_dem_stats).
constexpr int FRAME_G = 128;
constexpr int FRAME_PITCH = ROW + 1;

__global__ __launch_bounds__(FRAME_G) void k_dem_frame(DemTableView T, double* __restrict__ rows, double* __restrict__ addends) {
  __shared__ double lds[FRAME_G * FRAME_PITCH];
  const int n = T.n;
  const int g0 = blockIdx.x * FRAME_G;
  const int i = g0 + threadIdx.x;
  if (i < n) {
    const double x1 = T.K.x1[i], x2 = T.K.x2[i], x3 = T.K.x3[i], v1 = T.K.v1[i], v2 = T.K.v2[i], v3 = T.K.v3[i];
    const double a1 = T.K.a1[i], a2 = T.K.a2[i], a3 = T.K.a3[i];
    const double r = T.r[i], m = T.m[i], It = T.It[i], pp = T.gp[i];
    const size_t sn = (size_t)n;
    const double ss = T.diag[i], f1 = T.diag[sn + i], f2 = T.diag[2 * sn + i], ifm = T.diag[3 * sn + i];
    const int* zi = reinterpret_cast<const int*>(T.diag + 8 * sn);
    const int z = zi[i], zz = zi[sn + i];
    const double fr = T.fr[i], ice = T.ice[i], slip = T.slip[i], rw = T.rw[i];
    const double fm = (z == 0) ? 0. : ifm / z;                                                               // main.c:409-412
    const double ifr = fabs(((m * T.G + f2) * (T.dt * v2 + T.dt2 * a2 / 2.)) + (f1 * (T.dt * v1 + T.dt2 * a1 / 2.)));   // main.c:388-390
    const double ESE = 0.5 * (((pp * pp) / T.kg) + ((ss * ss) / T.kt));
    double* a = addends + i;
    a[0] = 0.5 * m * v1 * v1;
    a[sn] = 0.5 * m * v2 * v2;
    a[2 * sn] = 0.5 * It * v3 * v3;
    a[3 * sn] = m * T.G * x2;
    a[4 * sn] = ESE;
    a[5 * sn] = fr; a[6 * sn] = ifr; a[7 * sn] = ice; a[8 * sn] = slip; a[9 * sn] = rw;
    if (rows) {
      double* o = lds + threadIdx.x * FRAME_PITCH;
      o[0] = r; o[1] = x1; o[2] = x2; o[3] = x3; o[4] = v1; o[5] = v2; o[6] = v3; o[7] = a1; o[8] = a2; o[9] = a3;
      o[10] = T.fhf[i]; o[11] = T.fhf[sn + i]; o[12] = T.fhf[2 * sn + i];
      o[13] = pp; o[14] = ss; o[15] = ESE; o[16] = fr; o[17] = ifr; o[18] = ice; o[19] = slip; o[20] = rw; o[21] = fm;
      o[22] = T.diag[4 * sn + i]; o[23] = T.diag[5 * sn + i]; o[24] = T.diag[6 * sn + i]; o[25] = T.diag[7 * sn + i];
      o[26] = z; o[27] = zz;
    }
  }
  if (!rows) return;   // (uniform over the grid)
  __syncthreads();
  const int here = n - g0 < FRAME_G ? n - g0 : FRAME_G;
  double* out = rows + (size_t)g0 * ROW;
  for (int e = threadIdx.x; e < here * ROW; e += FRAME_G) out[e] = lds[(e / ROW) * FRAME_PITCH + e % ROW];
}

// ---- k_dem_stats: ONE workgroup -------------------------------------------------------------------------------------------------
// The ten floating-point sums are serial chains in grain order on the host and stay so here: lane c < 10 of the first wavefront
// adds up chain c, one grain after the other, from LDS. All 256 lanes fetch the addends a chunk of STATS_CH grains ahead
// (global -> registers while the chains run over the chunk before, registers -> the other LDS buffer afterwards), so the
// only thing a chain's add waits for is the add before it (the LDS reads run a group of eight grains ahead). The pitch of STATS_CH + 1 doubles puts the ten lanes' reads of
// one grain into ten different banks. The integer counts (z, N[0..5]) and the three maxima do not depend on the order:
// every lane takes a stride of the grains, lane 0 folds the 256 partial results.
constexpr int STATS_T = 256;
constexpr int STATS_CH = 256;
constexpr int STATS_PITCH = STATS_CH + 1;
static_assert(STATS_CH == STATS_T, "one addend per chain, lane and chunk");

__global__ __launch_bounds__(STATS_T) void k_dem_stats(DemTableView T, const double* __restrict__ addends, double* __restrict__ stats22) {
  __shared__ double buf[2][NCHAIN * STATS_PITCH];
  __shared__ double mx[3][STATS_T];
  __shared__ long long cnt[7][STATS_T];
  const int n = T.n, t = threadIdx.x;
  const size_t sn = (size_t)n;
  // order-free part
  {
    const int* zi = reinterpret_cast<const int*>(T.diag + 8 * sn);
    double xgrainmax = T.K.x1[0], height = T.K.x2[0] + T.r[0], xfront = T.K.x1[0] + T.r[0];   // main.c:352-354
    long long zsum = 0, N[6] = {0, 0, 0, 0, 0, 0};
    for (int i = t; i < n; i += STATS_T) {
      const double x1 = T.K.x1[i], x2 = T.K.x2[i], r = T.r[i];
      const int z = zi[i], zz = zi[sn + i];
      zsum += z;
#pragma unroll
      for (int k = 0; k < 6; ++k) N[k] += (z == k);
      if (x1 + r > xgrainmax) xgrainmax = x1 + r;
      if (x2 + r > height) height = x2 + r;
      if (zz > 0 && x1 + r >= xfront) xfront = x1 + r;
    }
    mx[0][t] = xfront; mx[1][t] = xgrainmax; mx[2][t] = height;
    cnt[0][t] = zsum;
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[1 + k][t] = N[k];
  }
  // the chains
  const int chunks = (n + STATS_CH - 1) / STATS_CH;
  double reg[NCHAIN];
  auto fetch = [&](int k) {
    const int i = k * STATS_CH + t;
#pragma unroll
    for (int c = 0; c < NCHAIN; ++c) reg[c] = i < n ? addends[c * sn + i] : 0.;
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int c = 0; c < NCHAIN; ++c) buf[b][c * STATS_PITCH + t] = reg[c];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  double acc = 0.;
  for (int k = 0; k < chunks; ++k) {
    if (k + 1 < chunks) fetch(k + 1);
    if (t < NCHAIN) {
      const double* a = &buf[k & 1][t * STATS_PITCH];
      const int here = n - k * STATS_CH < STATS_CH ? n - k * STATS_CH : STATS_CH;
      // groups of eight: the LDS reads of the next group are in flight while this group's adds run
      const int full = here & ~7;
      int j = 0;
      if (full) {
        double cur[8], nxt[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cur[u] = a[u];
        for (; j + 8 < full; j += 8) {
#pragma unroll
          for (int u = 0; u < 8; ++u) nxt[u] = a[j + 8 + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) acc += cur[u];
#pragma unroll
          for (int u = 0; u < 8; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += cur[u];
        j = full;
      }
      for (; j < here; ++j) acc += a[j];
    }
    if (k + 1 < chunks) stage((k + 1) & 1);
    __syncthreads();   // chunk k + 1 is staged, and nobody reads chunk k any more
  }
  __shared__ double sums[NCHAIN];
  if (t < NCHAIN) sums[t] = acc;
  __syncthreads();
  if (t != 0) return;
  double xfront = mx[0][0], xgrainmax = mx[1][0], height = mx[2][0];
  long long zsum = cnt[0][0], N[6];
  for (int k = 0; k < 6; ++k) N[k] = cnt[1 + k][0];
  for (int l = 1; l < STATS_T; ++l) {
    if (mx[0][l] > xfront) xfront = mx[0][l];
    if (mx[1][l] > xgrainmax) xgrainmax = mx[1][l];
    if (mx[2][l] > height) height = mx[2][l];
    zsum += cnt[0][l];
    for (int k = 0; k < 6; ++k) N[k] += cnt[1 + k][l];
  }
  const double energie_x = sums[0], energie_y = sums[1], energie_teta = sums[2];
  stats22[0] = 0.;   // nbsteps * dt - dtt: the host's
  stats22[1] = xfront; stats22[2] = xgrainmax; stats22[3] = height;
  stats22[4] = (double)zsum / n;
  stats22[5] = energie_x; stats22[6] = energie_y; stats22[7] = energie_teta;
  stats22[8] = energie_x + energie_y + energie_teta;
  for (int k = 0; k < 6; ++k) stats22[9 + k] = (double)N[k] / n;
  stats22[15] = sums[3]; stats22[16] = sums[4]; stats22[17] = sums[5]; stats22[18] = sums[6];
  stats22[19] = sums[7]; stats22[20] = sums[8]; stats22[21] = sums[9];
}

}  // namespace

void launch_dem_frame(const DemTableView& T, double* rows, double* addends, hipStream_t st) {
  hipLaunchKernelGGL(k_dem_frame, dim3((T.n + FRAME_G - 1) / FRAME_G), dim3(FRAME_G), 0, st, T, rows, addends);
}

void launch_dem_stats(const DemTableView& T, const double* addends, double* stats22, hipStream_t st) {
  hipLaunchKernelGGL(k_dem_stats, dim3(1), dim3(STATS_T), 0, st, T, addends, stats22);
}

#endif  // !LBMDEM_SINGLE_PRECISION
