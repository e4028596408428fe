// lbm_stage.h -- what the host halves of the map-reading analyses share (lbm_pores.hip, lbm_clearance.hip, lbm_network.hip,
// lbm_drainage.hip, lbm_geodesic.hip, lbm_netflux.hip, lbm_netsolve.hip): the stamp that says which map a result describes, the
// check and the upload of a caller's map, the download of a plane and of a table, the refusals of arguments several of them take,
// and the two files every one of them writes alike, the VTK of int planes and the run row of <stage>.data. Plain functions over
// the handle and OutFile; the computes, the kernels and the texts of the *_ready refusals stay with their stages. Host only.
#pragma once

#include "lbm_outfile.h"
#include "lbmdem_handle.h"

#include <limits.h>

#include <vector>

// MapStamp (lbmdem_handle.h): the map and the populations as they are now
inline void MapStamp::set(const lbmdem_handle* h) {
  seq = h->substep_seq; moved = h->grains_moved; fluid = h->lattice_seq;
  valid = true;
}
inline bool MapStamp::current(const lbmdem_handle* h) const {
  return valid && seq == h->substep_seq && moved == h->grains_moved && fluid == h->lattice_seq;
}

static inline long stage_blocks(long items, int per) { return (items + per - 1) / per; }
// bits that hold 0 .. v
static inline int stage_bits(unsigned long long v) { int b = 1; while (b < 64 && (v >> b)) ++b; return b; }
static inline unsigned stage_be32(int v) { return __builtin_bswap32((unsigned)v); }

// a caller's map (null: the handle's own, nothing to check): every entry -1, a grain or the wall
static inline int stage_check_map(const char* who, const int* map, int lx, int ly, int n) {
  if (map)
    for (long k = 0, cnt = (long)lx * ly; k < cnt; ++k)
      if (map[k] < -1 || map[k] > n)
        return fail(LBMDEM_EINVAL, "%s: map[%ld] = %d (node %ld, %ld) is neither -1 (fluid), a grain (0 .. %d) nor the wall (%d)",
                    who, k, map[k], k / ly, k % ly, n - 1, n);
  return LBMDEM_OK;
}
// ... into *slot in device layout (allocated by the first call that brings one): host rows of ly into device rows of sy, the pad
// columns are never read. Enqueues on the handle's stream; `map` is read until the caller's next synchronisation.
static inline int stage_upload_map(lbmdem_handle* h, int** slot, const int* map) {
  const LatticeView& L = h->L;
  if (!*slot) HIP_TRY(h->mem.dev(slot, (size_t)L.lx * L.sy));
  HIP_TRY(hipMemcpy2DAsync(*slot, sizeof(int) * L.sy, map, sizeof(int) * L.ly, sizeof(int) * L.ly, L.lx, hipMemcpyHostToDevice,
                           h->stream));
  return LBMDEM_OK;
}
// a result plane into host rows of ly; enqueues only, the caller synchronises
static inline int stage_download_plane(lbmdem_handle* h, int* out, const int* src) {
  const LatticeView& L = h->L;
  HIP_TRY(hipMemcpy2DAsync(out, sizeof(int) * L.ly, src, sizeof(int) * L.sy, sizeof(int) * L.ly, L.lx, hipMemcpyDeviceToHost,
                           h->stream));
  return LBMDEM_OK;
}
// a table of `have` records of `each` bytes on the device: cap = 0 reports *count, a short buffer is refused with *count set and
// nothing written, else the records are copied and the stream is synchronised
static inline int stage_table(lbmdem_handle* h, const char* who, const char* what, const void* src, size_t each, long have,
                              void* out, long cap, long* count) {
  *count = have;
  if (cap == 0) return LBMDEM_OK;   // (how many there are)
  if (cap < have) return fail(LBMDEM_EINVAL, "%s: there are %ld %s, the buffer holds %ld", who, have, what, cap);
  if (have > 0) {
    HIP_TRY(hipMemcpyAsync(out, src, each * (size_t)have, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return LBMDEM_OK;
}

static inline int stage_check_max_edges(const char* who, long max_edges) {
  if (max_edges < 0 || max_edges > (long)INT_MAX)
    return fail(LBMDEM_EINVAL, "%s: max_edges must lie in 0 .. %d (%ld)", who, INT_MAX, max_edges);
  return LBMDEM_OK;
}
// the masks of the inlet and outlet sides and the band behind them; need_to: the stage has no meaning without an outlet, so
// to == 0 is refused too, in a sentence of its own (the test behind it cannot fire then: need_to changes the sentence only)
static inline int stage_check_sides(const char* who, int from, int band, int to, bool need_to = false) {
  if (from < 1 || from > 15)
    return fail(LBMDEM_EINVAL, "%s: from must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (%d)", who, from);
  if (need_to && (to < 1 || to > 15))
    return fail(LBMDEM_EINVAL, "%s: to must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one (%d)", who, to);
  if (to < 0 || to > 15)
    return fail(LBMDEM_EINVAL, "%s: to must be a mask of sides, B 1 | T 2 | L 4 | R 8, or 0 for no outlet (%d)", who, to);
  if (band < 1) return fail(LBMDEM_EINVAL, "%s: band must be at least 1 node (%d)", who, band);
  return LBMDEM_OK;
}

// <dir>/<file_fmt % nfile>: a binary STRUCTURED_POINTS VTK of `count` int planes in host layout ([lx][ly], written as big-endian
// images of ly rows); newline_after: a line feed behind every plane's image. -> F.close(a write was short)
static inline int stage_write_int_planes(OutFile& F, const char* dir, int nfile, const char* file_fmt, const char* title, int lx,
                                         int ly, const char* const* names, const int* const* planes, int count,
                                         bool newline_after = true) {
  const size_t cnt = (size_t)lx * ly;
  std::vector<unsigned> image(cnt);
  const float pas = (float)(1. / lx);   // (lbmdem_vtk_put_mesh's)
  RC_TRY(F.open("w+", dir, file_fmt, nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# vtk DataFile Version 2.0\n%s\nBINARY\nDATASET STRUCTURED_POINTS\n", title);
  fprintf(fp, "DIMENSIONS %d %d 1\nORIGIN 0 0 0\nSPACING %.9g %.9g 1\n", lx, ly, (double)pas, (double)pas);
  fprintf(fp, "POINT_DATA %ld\n", (long)cnt);
  bool short_write = false;
  for (int k = 0; k < count; ++k) {
    for (int y = 0; y < ly; ++y)
      for (int x = 0; x < lx; ++x) image[(size_t)y * lx + x] = stage_be32(planes[k][(size_t)x * ly + y]);
    fprintf(fp, "SCALARS %s int 1\nLOOKUP_TABLE default\n", names[k]);
    short_write = short_write || fwrite(image.data(), 4, cnt, fp) != cnt;
    if (newline_after) fprintf(fp, "\n");
  }
  return F.close(short_write);
}
// the run's row of <dir>/<file>: t, the counts and the sums; `header` goes first into an empty file
static inline int stage_append_row(OutFile& F, const char* dir, const char* file, const char* header, double t, const long* counts,
                                   int ncounts, const double* sums = nullptr, int nsums = 0) {
  RC_TRY(F.open("a", dir, "%s", file));
  FILE* fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0) fprintf(fp, "%s\n", header);
  fprintf(fp, "%le", t);
  for (int k = 0; k < ncounts; ++k) fprintf(fp, " %ld", counts[k]);
  for (int k = 0; k < nsums; ++k) fprintf(fp, " %.17g", sums[k]);
  fprintf(fp, "\n");
  return F.close();
}
