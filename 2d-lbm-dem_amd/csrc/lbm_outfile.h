// lbm_outfile.h -- one checked output file for the writers that report through fail(): the text and VTK files of the exports
// (lbm_links.hip, lbm_densities.hip, lbm_contacts.hip, lbm_clusters.hip: clusters.data too, lbm_structure.hip: structure.data too, lbm_voronoi.hip: voronoi.data too, lbm_strain.hip: strain.data too, the seven map-reading analyses of lbm_stage.h, whose VTK planes and <stage>.data rows that header writes, lbm_coarse.hip, lbm_flow.hip, lbm_tracers.hip, lbm_scalar.hip: scalar.data too, lbm_mean.hip) and flow.data (lbmdem_scene.hip). Host only.
// The writers of lbmdem_output.hip are not meant: they report into a buffer for the writer thread and say why a write failed.
#pragma once

#include "lbmdem_handle.h"

struct OutFile {   // not copyable; an early return closes the file quietly
  FILE* fp = nullptr;
  char path[4300];
  OutFile() = default;
  OutFile(const OutFile&) = delete;
  OutFile& operator=(const OutFile&) = delete;
  ~OutFile() { if (fp) fclose(fp); }

  // <dir>/<name>, the name printf style; no directory is "."
  int open(const char* mode, const char* dir, const char* name, ...) __attribute__((format(printf, 4, 5))) {
    int at = snprintf(path, sizeof path, "%s/", (dir && *dir) ? dir : ".");
    if (at < 0 || (size_t)at >= sizeof path) at = (int)sizeof path - 1;
    va_list ap;
    va_start(ap, name);
    vsnprintf(path + at, sizeof path - (size_t)at, name, ap);
    va_end(ap);
    fp = fopen(path, mode);
    if (!fp) return fail(LBMDEM_EINVAL, "cannot open '%s' for writing", path);
    return LBMDEM_OK;
  }
  // closes; true when the stream had an error or the close failed (for a caller with a text of its own)
  bool finish() {
    bool bad = ferror(fp) != 0;
    bad |= fclose(fp) != 0;
    fp = nullptr;
    return bad;
  }
  // closes; `bad`: what else the caller knows to have gone wrong (a short fwrite)
  int close(bool bad = false) {
    if (finish() || bad) return fail(LBMDEM_EINVAL, "writing '%s' failed", path);
    return LBMDEM_OK;
  }
};
