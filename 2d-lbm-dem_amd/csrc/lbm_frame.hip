// lbm_frame.hip -- one VTK frame as the files hold it: the five point-data payloads of write_vtk (main.c:284-323) back to
// back, big-endian float32 -- grain_pressure[ly][nx], grain_velocity[ly][nx][3], grain_acceleration[ly][nx][3],
// fluid_pressure[ly][nx], fluid_velocity[ly][nx][3] (nx = owned rows), 44 bytes per node. The arithmetic is k_vtk_fields'
// (lbm_lattice.hip), statement for statement; only the memory side differs.

#include "lbm_device.h"

namespace {

// A workgroup owns FRAME_BX lattice rows x one y-tile of the population layout (64 x 16 nodes in the double build, 32 x 32
// in the float build: 1 024 nodes, four per lane, either way).
//   in:  lanes run along y first -- f[x][y / T][q][y % T] and obst[x][y] have y as the fast axis: a tile's nine directions
//        are nine consecutive 128-byte lines per x, every line used whole;
//   LDS: the eight floats a node yields (grain pressure, 2 x velocity, 2 x acceleration, fluid pressure, 2 x fluid
//        velocity; the third components are constants), plane by plane, [y][x] with a padded pitch;
//   out: lanes run along x first -- the files are [y][x]: runs of 4 FRAME_BX bytes for the scalars, 12 FRAME_BX for the
//        interleaved vectors, already byte-swapped (__builtin_bswap32 on the bit pattern), 4-byte vector stores.
// LDS banking of the 4-byte accesses (32 banks, lane groups of 32): a group writes 32 / T columns x T rows at
// y * PITCH + x -- PITCH = 2 (mod 32) for T = 16, odd for T = 32 keeps them apart; a group reads 32 consecutive elements of an
// output row, i.e. 32 x of one plane or ~11 x of two planes: PLANE = 16 (mod 32) keeps the two planes apart.
constexpr int FRAME_TY = LBMDEM_TILE_Y;
constexpr int FRAME_BX = 1024 / FRAME_TY;
constexpr int FRAME_PITCH = FRAME_BX + (FRAME_TY == 16 ? 2 : 1);
constexpr int FRAME_PLANE = FRAME_TY * FRAME_PITCH + 16;
static_assert((FRAME_TY * FRAME_PITCH) % 32 == 0, "plane padding assumes this");

// one payload of the image: `dim` floats per node from planes p0, p0 + 1 (dim == 3: the third is 0.f)
template <int DIM>
__device__ __forceinline__ void frame_store(const float* __restrict__ lds, int p0, unsigned* __restrict__ out, int nx, int ly,
                                            int x0, int y0) {
  constexpr int ROW = FRAME_BX * DIM;
#pragma unroll
  for (int it = 0; it < FRAME_TY * ROW / 256; ++it) {
    const int e = it * 256 + threadIdx.x;
    const int yl = e / ROW, j = e % ROW, xl = j / DIM, comp = j % DIM;
    if (x0 + xl < nx && y0 + yl < ly) {
      const float v = comp < 2 ? lds[(p0 + comp) * FRAME_PLANE + yl * FRAME_PITCH + xl] : 0.f;
      out[((size_t)(y0 + yl) * nx + x0) * DIM + j] = __builtin_bswap32(__float_as_uint(v));
    }
  }
}

__global__ __launch_bounds__(256) void k_vtk_frame(const real* __restrict__ f, const int* __restrict__ obst, LatticeView L,
                                                   const real* __restrict__ gp, const real* __restrict__ v1,
                                                   const real* __restrict__ v2, const real* __restrict__ a1,
                                                   const real* __restrict__ a2, real rho_moy, unsigned* __restrict__ image) {
  __shared__ float lds[8 * FRAME_PLANE];
  const int nx = L.xo1 - L.xo0;
  const int x0 = blockIdx.x * FRAME_BX, y0 = blockIdx.y * FRAME_TY;
#pragma unroll
  for (int it = 0; it < FRAME_BX * FRAME_TY / 256; ++it) {
    const int idx = it * 256 + threadIdx.x;
    const int yl = idx % FRAME_TY, xl = idx / FRAME_TY;
    const int xr = x0 + xl, y = y0 + yl;
    if (xr >= nx || y >= L.ly) continue;
    const long node = (long)(L.xo0 + xr) * L.sy + y;
    const int i = obst[node];
    float gpr = -1.f, gv0 = 0.f, gv1 = 0.f, ga0 = 0.f, ga1 = 0.f, fp = 0.f, fv0 = 0.f, fv1 = 0.f;
    if (i >= 0 && i < L.n) {
      gpr = (float)gp[i];
      gv0 = (float)v1[i]; gv1 = (float)v2[i];
      ga0 = (float)a1[i]; ga1 = (float)a2[i];
    } else {
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const real v = f[fidx(q, node)];
        fp = (float)((real)fp + v);
        fv0 = (float)((real)fv0 + v * EXq(q));
        fv1 = (float)((real)fv1 + v * EYq(q));
      }
      fp = (float)((1. / 3.) * rho_moy * ((real)fp - 1.));
    }
    float* o = lds + yl * FRAME_PITCH + xl;
    o[0] = gpr;
    o[FRAME_PLANE] = gv0; o[2 * FRAME_PLANE] = gv1;
    o[3 * FRAME_PLANE] = ga0; o[4 * FRAME_PLANE] = ga1;
    o[5 * FRAME_PLANE] = fp;
    o[6 * FRAME_PLANE] = fv0; o[7 * FRAME_PLANE] = fv1;
  }
  __syncthreads();
  const size_t cnt = (size_t)nx * L.ly;
  frame_store<1>(lds, 0, image, nx, L.ly, x0, y0);
  frame_store<3>(lds, 1, image + cnt, nx, L.ly, x0, y0);
  frame_store<3>(lds, 3, image + 4 * cnt, nx, L.ly, x0, y0);
  frame_store<1>(lds, 5, image + 7 * cnt, nx, L.ly, x0, y0);
  frame_store<3>(lds, 6, image + 8 * cnt, nx, L.ly, x0, y0);
}

}  // namespace

void launch_vtk_frame(const real* f, const int* obst, const LatticeView& L, const real* gp, const real* v1, const real* v2,
                      const real* a1, const real* a2, real rho_moy, void* image_be, hipStream_t st) {
  const int nx = L.xo1 - L.xo0;
  hipLaunchKernelGGL(k_vtk_frame, dim3((nx + FRAME_BX - 1) / FRAME_BX, (L.ly + FRAME_TY - 1) / FRAME_TY), dim3(256), 0, st, f,
                     obst, L, gp, v1, v2, a1, a2, rho_moy, static_cast<unsigned*>(image_be));
}
