// lbmdem_checkpoint.hip -- checkpoint / restart of a handle (the reference cannot resume a run): single domain, or one
// file per rank of a strip decomposition with distributed grains; the digest trailer of the checkpoints written in the
// background (lbmdem_checkpoint_save_async, lbmdem_output.hip), its verifier, and the cadence setting of lbmdem_run_scene.

#include "lbmdem_handle.h"

#include <errno.h>
#include <sys/stat.h>

#pragma GCC visibility push(default)
extern "C" {
// ---- checkpoint / restart ------------------------------------------------------------------------

namespace {
struct CkptHeader {
  char magic[8];       // "LBMDEMC5"
  double lid6;         // lbmdem_set_lid
  int layout;          // device layout of the populations in the file: 1 = 16-node tiles f[x][y/16][q][y%16]
  int force_mode, diag_always, has_carry;
  double carry[3];     // pft, pff, pf of the order-dependent contact diagnostics (main.c:130-131), when has_carry
  lbmdem_config cfg;   // incl. the wall positions VerletWall may have moved
  long nbsteps;
  int verlet_ok, nnbr; // symmetric list length
  long plane;          // sanity: nxl * sy of the writer
  int has_dist;        // a CkptDist section follows the lattice (the writer had its grains distributed over strips)
  int vib;             // 1: the walls vibrate (lbmdem_set_vibration; t, Mgx, Mdx are in cfg). 0 in every other file
};
struct CkptDist {       // follows the lattice when the writer had its grains distributed over strips
  char magic[8];        // "LBMDIST1"
  int margin, cap_g, cap_t, cap_l, poison, pad;
};
constexpr int CKPT_LAYOUT = 1;
static bool wr(FILE* fp, const void* p, size_t n) { return fwrite(p, 1, n, fp) == n; }
static bool rd(FILE* fp, void* p, size_t n) { return fread(p, 1, n, fp) == n; }
struct FileCloser {   // closes on every exit path, exceptions included
  FILE* fp;
  ~FileCloser() { if (fp) fclose(fp); }
};
static bool header_plausible(const CkptHeader& H) {
  const lbmdem_config& hc = H.cfg;
  return !(hc.nbgrains < 1 || hc.nbgrains > (1 << 28) || hc.lx < 3 || hc.ly < 3 || hc.lx > (1 << 24) || hc.ly > (1 << 24) ||
           hc.x_begin < 0 || hc.x_end > hc.lx || hc.x_begin >= hc.x_end || hc.halo < 0 || hc.halo > hc.lx || hc.npDEM < 1 ||
           H.nnbr < 0 || H.nbsteps < 0 || H.plane < 1 || (H.has_dist != 0 && H.has_dist != 1) || (H.vib != 0 && H.vib != 1));
}

// ---- the digest trailer ("LBMCKSM1") --------------------------------------------------------------------------------------
// Behind everything lbmdem_checkpoint_save writes: magic, int nsections, int 0, then {bytes, S1, S2} per section in file order.
// Every byte in front of the trailer belongs to exactly one section; the header is its own first section.
typedef unsigned long long u64;
constexpr int CKSM_SECTIONS = 1 + CKPT_DEV_SECTIONS;
static const char* const CKSM_NAMES[CKSM_SECTIONS] = {"header", "r", "kin", "fhf", "gp", "offsets", "nbr", "wallflags", "obst", "f"};
struct CksmEntry { u64 bytes, s1, s2; };
struct CksmTrailer {
  char magic[8];
  int nsections, pad;
  CksmEntry e[CKSM_SECTIONS];
};
static_assert(sizeof(CksmTrailer) == 16 + 24 * CKSM_SECTIONS, "the trailer has no padding");

// THE digest routine (the writer thread, the verifier, lbmdem_checkpoint_digest): `nbytes` bytes that begin at word
// `first_word` of their section are added to acc = {S1, S2}; a piece that ends inside a word ends the section (zero-padded)
static void digest_add(const void* bytes, size_t nbytes, u64 first_word, u64 acc[2]) {
  const unsigned char* p = static_cast<const unsigned char*>(bytes);
  u64 s1 = acc[0], s2 = acc[1], i = first_word;
  size_t k = 0;
  for (; k + 8 <= nbytes; k += 8, ++i) {
    u64 w;
    memcpy(&w, p + k, 8);   // (the library runs on little-endian hosts only)
    s1 += w;
    s2 += (i + 1) * w;
  }
  if (k < nbytes) {
    u64 w = 0;
    memcpy(&w, p + k, nbytes - k);
    s1 += w;
    s2 += (i + 1) * w;
  }
  acc[0] = s1; acc[1] = s2;
}

// the lengths of the ten sections of a file with this header
static void section_lengths(const CkptHeader& H, u64 len[CKSM_SECTIONS]) {
  const CkptLayout Y = ckpt_layout(H.cfg.nbgrains, H.nnbr, H.plane);
  len[0] = sizeof(CkptHeader);
  for (int s = 0; s < CKPT_DEV_SECTIONS; ++s) len[1 + s] = Y.bytes[s];
}

// lbmdem_checkpoint_verify. A trailer is looked for where a complete file has it, at the very end: its presence does not hang
// on a header that may itself be damaged, and the header is then the first section checked. A file that ends differently
// has a trailer only if one begins right behind the sections its header announces -- cut short, then. `lenient`
// (lbmdem_checkpoint_load's use): a file WITHOUT a trailer whose header cannot be read, or that is shorter than its header
// claims, passes -- the loader's own checks and messages follow, as before.
static int verify_file(const char* path, int* has_digest, bool lenient) {
  *has_digest = 0;
  FILE* fp = fopen(path, "rb");
  if (!fp) return lenient ? LBMDEM_OK : fail(LBMDEM_EINVAL, "cannot open checkpoint '%s'", path);
  FileCloser closer{fp};
  struct stat stt{};
  if (fstat(fileno(fp), &stt) != 0) return lenient ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s': cannot take its size", path);
  const u64 size = (u64)stt.st_size;
  CkptHeader H;
  CksmTrailer T;
  memset(&T, 0, sizeof T);
  const bool at_end = size >= sizeof H + sizeof T && fseeko(fp, (off_t)(size - sizeof T), SEEK_SET) == 0 && rd(fp, &T, sizeof T) &&
                      memcmp(T.magic, "LBMCKSM1", 8) == 0;
  if (fseeko(fp, 0, SEEK_SET) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot rewind", path);
  const bool have_header = rd(fp, &H, sizeof H);
  if (at_end) {
    *has_digest = 1;
    u64 acc[2] = {0, 0};
    digest_add(&H, sizeof H, 0, acc);
    if (T.nsections != CKSM_SECTIONS || T.pad != 0 || T.e[0].bytes != sizeof H)
      return fail(LBMDEM_EINVAL, "checkpoint '%s': its digest trailer is malformed", path);
    if (!have_header || acc[0] != T.e[0].s1 || acc[1] != T.e[0].s2)
      return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'header' does not match its digest (the file is torn or corrupted)", path);
  }
  if (!have_header || memcmp(H.magic, "LBMDEMC5", 8) != 0 || H.layout != CKPT_LAYOUT || !header_plausible(H))
    return lenient && !at_end ? LBMDEM_OK : fail(LBMDEM_EINVAL, "'%s' is not a checkpoint of this library version", path);
  u64 len[CKSM_SECTIONS], fixed = 0;
  section_lengths(H, len);
  for (int s = 0; s < CKSM_SECTIONS; ++s) fixed += len[s];
  if (!at_end) {
    if (size < fixed) return lenient ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its header claims (%llu of at least %llu bytes)", path, size, fixed);
    const u64 rest = size - fixed;
    char head[8];
    const size_t k = rest < 8 ? (size_t)rest : 8;
    if (k == 0) return LBMDEM_OK;
    if (fseeko(fp, (off_t)fixed, SEEK_SET) != 0 || !rd(fp, head, k)) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot read behind its sections", path);
    if (memcmp(head, "LBMCKSM1", k) != 0) return LBMDEM_OK;   // (e.g. the strips' "LBMDIST1" section)
    *has_digest = 1;
    return fail(LBMDEM_EINVAL, "checkpoint '%s': its digest trailer is cut short (%llu of %zu bytes)", path, rest, sizeof T);
  }
  if (fixed + sizeof T != size)
    return fail(LBMDEM_EINVAL, "checkpoint '%s': %llu bytes by its header and digest trailer, %llu in the file", path, fixed + (u64)sizeof T, size);
  if (fseeko(fp, (off_t)sizeof H, SEEK_SET) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot seek", path);
  std::vector<unsigned char> buf((size_t)1 << 22);
  for (int s = 1; s < CKSM_SECTIONS; ++s) {
    if (T.e[s].bytes != len[s])
      return fail(LBMDEM_EINVAL, "checkpoint '%s': section '%s' is %llu bytes long by the header and %llu by the digest trailer", path,
                  CKSM_NAMES[s], len[s], T.e[s].bytes);
    u64 acc[2] = {0, 0};
    for (u64 done = 0; done < len[s];) {
      const size_t piece = len[s] - done < buf.size() ? (size_t)(len[s] - done) : buf.size();
      if (!rd(fp, buf.data(), piece)) return fail(LBMDEM_EINVAL, "checkpoint '%s': section '%s' cannot be read", path, CKSM_NAMES[s]);
      digest_add(buf.data(), piece, done / 8, acc);
      done += piece;
    }
    if (acc[0] != T.e[s].s1 || acc[1] != T.e[s].s2)
      return fail(LBMDEM_EINVAL, "checkpoint '%s': section '%s' does not match its digest (the file is torn or corrupted)", path, CKSM_NAMES[s]);
  }
  return LBMDEM_OK;
}
}  // namespace

#ifndef LBMDEM_SINGLE_PRECISION
// ---- checkpoints in the background: the two ends of a slot's way (the middle is lbmdem_output.hip's) --------------------------
void lbmdem_ckpt_frame_job(const lbmdem_handle* h, const CkptLayout& Y, unsigned char* staging, CkptFrameJob* J) {
  const void* src[CKPT_DEV_SECTIONS] = {h->r, h->kin[h->kcur].x1, h->fhf, h->gp, h->verlet_ok ? h->V.offsets : nullptr,
                                        h->V.nbr, h->V.wallflags, h->obst[h->ocur], h->f[h->fcur]};
  for (int s = 0; s < CKPT_DEV_SECTIONS; ++s) { J->src[s] = src[s]; J->bytes[s] = Y.bytes[s]; J->at[s] = Y.at[s]; }
  J->nnbr = h->verlet_ok ? h->V.offsets + h->n : nullptr;   // (lbmdem_checkpoint_save: zero offsets, no entries without a list)
  J->carry = h->ct.carry;
  J->staging = staging;
  J->gate = h->L.gate;
}

int lbmdem_ckpt_write_slot(const AsyncSlot* S, const CkptLayout* Y, char* msg, size_t msglen) {
  const unsigned char* image = static_cast<const unsigned char*>(S->pinned);
  const u64* words = reinterpret_cast<const u64*>(image);
  const CkptShot& C = S->shot;
  CkptHeader H;
  memset(&H, 0, sizeof H);
  memcpy(H.magic, "LBMDEMC5", 8);
  H.lid6 = C.lid6;
  H.layout = CKPT_LAYOUT; H.force_mode = C.force_mode; H.diag_always = C.diag_always;
  H.has_carry = 1;
  memcpy(H.carry, words + 1, sizeof H.carry);
  H.cfg = C.cfg; H.nbsteps = C.nbsteps; H.verlet_ok = C.verlet_ok; H.nnbr = (int)words[0]; H.plane = C.plane;
  H.has_dist = 0;
  H.vib = C.vib;
  CksmTrailer T;
  memset(&T, 0, sizeof T);
  memcpy(T.magic, "LBMCKSM1", 8);
  T.nsections = CKSM_SECTIONS;
  {
    u64 acc[2] = {0, 0};
    digest_add(&H, sizeof H, 0, acc);
    T.e[0] = CksmEntry{sizeof H, acc[0], acc[1]};
  }
  for (int s = 0; s < CKPT_DEV_SECTIONS; ++s) {
    const u64 bytes = s == CKPT_NBR ? 4 * (u64)H.nnbr : Y->bytes[s];
    T.e[1 + s] = CksmEntry{bytes, words[4 + 2 * s], words[5 + 2 * s]};
  }
  char tmp[sizeof S->path + 8];
  snprintf(tmp, sizeof tmp, "%s.tmp", S->path);
  FILE* fp = fopen(tmp, "wb");
  if (!fp) { snprintf(msg, msglen, "cannot open '%s' for writing: %s", tmp, strerror(errno)); return LBMDEM_EINVAL; }
  bool ok = wr(fp, &H, sizeof H);
  for (int s = 0; s < CKPT_DEV_SECTIONS && ok; ++s) ok = wr(fp, image + Y->at[s], (size_t)T.e[1 + s].bytes);   // exact lengths
  if (ok) ok = wr(fp, &T, sizeof T);
  int err = errno;
  if (fclose(fp) != 0) { if (ok) err = errno; ok = false; }
  if (ok && rename(tmp, S->path) != 0) { err = errno; ok = false; }
  if (!ok) {
    (void)remove(tmp);
    snprintf(msg, msglen, "writing checkpoint '%s' by way of '%s' failed: %s", S->path, tmp, strerror(err));
    return LBMDEM_EINVAL;
  }
  return LBMDEM_OK;
}
#endif

int lbmdem_checkpoint_save(lbmdem_handle* h, const char* path) try {
  SP_UNAVAILABLE("checkpointing");
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!path) return fail(LBMDEM_EINVAL, "null path");
  if (h->obst_pending) return fail(LBMDEM_EINVAL, "checkpoint between obst_construction and collide_stream");
  // (a handle with distributed grains writes ITS strip, the grains as it holds them, its ownership masks and message
  // capacities: one file per rank; the carries must have been agreed over the ranks first, lbmdem_comm_sync_carries)
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int n = h->n;
  std::vector<int> off(n + 1, 0);
  if (h->verlet_ok) HIP_TRY(hipMemcpy(off.data(), h->V.offsets, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
  CkptHeader H;
  memset(&H, 0, sizeof H);
  memcpy(H.magic, "LBMDEMC5", 8);
  H.lid6 = h->L.lid6;
  H.layout = CKPT_LAYOUT; H.force_mode = h->force_mode; H.diag_always = h->diag_always ? 1 : 0;
  H.has_carry = 1;
  if (!h->dist && h->carry_from < h->substep_seq) {
    launch_carry_resolve(h->ct, h->carry_from, h->stream);
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  HIP_TRY(hipMemcpy(H.carry, h->ct.carry, sizeof H.carry, hipMemcpyDeviceToHost));
  H.cfg = h->cfg; H.nbsteps = h->nbsteps; H.verlet_ok = h->verlet_ok ? 1 : 0; H.nnbr = off[n]; H.plane = h->L.plane;
  H.has_dist = h->dist ? 1 : 0;
  H.vib = h->vib ? 1 : 0;
  FILE* fp = fopen(path, "wb");
  if (!fp) return fail(LBMDEM_EINVAL, "cannot open '%s' for writing", path);
  bool ok = wr(fp, &H, sizeof H);
  auto dump = [&](const void* dev, size_t bytes) {
    if (!ok || bytes == 0) return;
    std::vector<char> buf(bytes);
    if (hipMemcpy(buf.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) { ok = false; return; }
    ok = wr(fp, buf.data(), bytes);
  };
  dump(h->r, sizeof(double) * n);
  dump(h->kin[h->kcur].x1, sizeof(double) * 9 * n);
  dump(h->fhf, sizeof(double) * 3 * n);
  dump(h->gp, sizeof(double) * n);
  dump(h->V.offsets, sizeof(int) * (n + 1));
  dump(h->V.nbr, sizeof(int) * (size_t)H.nnbr);
  dump(h->V.wallflags, n);
  dump(h->obst[h->ocur], sizeof(int) * (size_t)h->L.plane);
  for (int q = 0; q < 9 && ok; ++q)  // the lattice (device layout) in nine chunks: bounded host staging
    dump(h->f[h->fcur] + (size_t)q * h->L.plane, sizeof(double) * (size_t)h->L.plane);
  if (h->dist && ok) {   // optional trailing section
    CkptDist D;
    memset(&D, 0, sizeof D);
    memcpy(D.magic, "LBMDIST1", 8);
    D.margin = h->dist_margin; D.cap_g = h->dd.cap_g; D.cap_t = h->dd.cap_t; D.cap_l = h->dd.cap_l;
    D.poison = h->dist_poison ? 1 : 0;
    ok = wr(fp, &D, sizeof D);
    dump(h->dd.active, n); dump(h->dd.fluidmask, n); dump(h->owner, n);
  }
  ok = (fclose(fp) == 0) && ok;
  if (!ok) return fail(LBMDEM_EHIP, "writing checkpoint '%s' failed", path);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

int lbmdem_checkpoint_load(const char* path, int device, lbmdem_handle** out) try {
  SP_UNAVAILABLE("checkpointing");
  if (!path || !out) return fail(LBMDEM_EINVAL, "null argument");
  *out = nullptr;
  {   // a file that carries digests (lbmdem_checkpoint_save_async) is checked against them before anything else is done with it
    int has_digest = 0;
    RC_TRY(verify_file(path, &has_digest, true));
  }
  FILE* fp = fopen(path, "rb");
  if (!fp) return fail(LBMDEM_EINVAL, "cannot open checkpoint '%s'", path);
  FileCloser closer{fp};
  CkptHeader H;
  if (!rd(fp, &H, sizeof H) || memcmp(H.magic, "LBMDEMC5", 8) != 0) return fail(LBMDEM_EINVAL, "'%s' is not a checkpoint of this library version", path);
  if (H.layout != CKPT_LAYOUT) return fail(LBMDEM_EINVAL, "checkpoint '%s' holds another device layout (%d)", path, H.layout);
  // the header is not trusted: sizes are checked before anything is allocated from them
  const lbmdem_config& hc = H.cfg;
  if (!header_plausible(H))
    return fail(LBMDEM_EINVAL, "checkpoint '%s': implausible header (grains %d, lattice %d x %d, rows [%d, %d))", path,
                hc.nbgrains, hc.lx, hc.ly, hc.x_begin, hc.x_end);
  const int n = H.cfg.nbgrains;
  {   // nothing is allocated from a header the file itself cannot back: the fixed part alone is this long
    struct stat stt{};
    const long long need = (long long)sizeof H + (long long)sizeof(double) * 14 * n + (long long)sizeof(int) * (n + 1) +
                           (long long)sizeof(int) * H.nnbr + n + (long long)(sizeof(int) + 9 * sizeof(double)) * H.plane;
    if (fstat(fileno(fp), &stt) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot take its size (at least %lld bytes needed)", path, need);
    if ((long long)stt.st_size < need)
      return fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its header claims (%lld of at least %lld bytes)", path,
                  (long long)stt.st_size, need);
  }
  std::vector<double> r(n), kin(9 * (size_t)n);
  if (!rd(fp, r.data(), sizeof(double) * n) || !rd(fp, kin.data(), sizeof(double) * 9 * n)) return fail(LBMDEM_EINVAL, "checkpoint truncated");
  lbmdem_config cfg = H.cfg;
  cfg.device = device;
  lbmdem_handle* h = nullptr;
  int rc = lbmdem_create(&cfg, r.data(), kin.data(), kin.data() + n, &h);  // x1, x2 are the first two columns
  if (rc != LBMDEM_OK) return rc;
  struct HandleGuard {   // whatever leaves this function early -- a return, a bad_alloc in a staging buffer -- frees the handle
    lbmdem_handle* h;
    ~HandleGuard() { if (h) lbmdem_destroy(h); }
  } guard{h};
  bool ok = h->L.plane == H.plane && H.nnbr <= h->V.cap;
  auto fill = [&](void* dev, size_t bytes) {
    if (!ok || bytes == 0) return;
    std::vector<char> buf(bytes);
    ok = rd(fp, buf.data(), bytes) && hipMemcpy(dev, buf.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (ok) ok = hipMemcpy(h->kin[0].x1, kin.data(), sizeof(double) * 9 * n, hipMemcpyHostToDevice) == hipSuccess;
  h->kcur = 0;
  fill(h->fhf, sizeof(double) * 3 * n);
  fill(h->gp, sizeof(double) * n);
  {   // the pair list goes straight into kernels that index with it: checked here, on the host
    std::vector<int> off((size_t)n + 1), nb((size_t)H.nnbr);
    if (ok) ok = rd(fp, off.data(), sizeof(int) * off.size()) && rd(fp, nb.data(), sizeof(int) * nb.size());
    if (ok && H.verlet_ok) {
      ok = off[0] == 0 && off[n] == H.nnbr;
      for (int i = 0; i < n && ok; ++i) ok = off[i] <= off[i + 1];
      for (long k = 0; k < H.nnbr && ok; ++k) ok = nb[k] >= 0 && nb[k] < n;
      if (!ok) return fail(LBMDEM_EINVAL, "checkpoint '%s': the pair list is inconsistent", path);
    }
    if (ok) ok = hipMemcpy(h->V.offsets, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice) == hipSuccess &&
                 (H.nnbr == 0 || hipMemcpy(h->V.nbr, nb.data(), sizeof(int) * nb.size(), hipMemcpyHostToDevice) == hipSuccess);
    // the per-grain counts the offsets are the running sum of (a rebuild leaves both; the last grain's total is formed from them)
    std::vector<int> cnt((size_t)n);
    for (int i = 0; i < n && ok; ++i) cnt[i] = off[i + 1] - off[i];
    if (ok) ok = hipMemcpy(h->V.counts, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice) == hipSuccess;
  }
  fill(h->V.wallflags, n);
  fill(h->obst[0], sizeof(int) * (size_t)h->L.plane);
  h->ocur = 0; h->obst_pending = false;
  h->chg_state[0] = h->chg_state[1] = 0;
  h->snap_ok[0] = h->snap_ok[1] = false;   // (the loaded map is not the picture lbmdem_create has just painted)
  h->geo_buf = -1;                         // (... nor do the centres of that paint describe it)
  for (int q = 0; q < 9 && ok; ++q) fill(h->f[0] + (size_t)q * h->L.plane, sizeof(double) * (size_t)h->L.plane);
  h->fcur = 0;
  if (ok && H.has_dist) {   // a strip with distributed grains: masks and message capacities as the writer had them. A
    CkptDist D;             // missing or short section fails the load HERE, not later inside a collective on one rank
    ok = rd(fp, &D, sizeof D) && memcmp(D.magic, "LBMDIST1", 8) == 0 && D.margin > 0 && D.cap_g > 0 && D.cap_t > 0 &&
         D.cap_l > 0 && D.cap_g <= n && D.cap_t <= n && D.cap_l <= n &&
         lbmdem_dist_enable_caps(h, D.margin, D.cap_g, D.cap_t, D.cap_l) == LBMDEM_OK;
    if (ok) { fill(h->dd.active, n); fill(h->dd.fluidmask, n); fill(h->owner, n); h->dist_poison = D.poison != 0; }
  }
  if (!ok) return fail(LBMDEM_EINVAL, "checkpoint '%s' is truncated or from a different decomposition", path);
  h->cfg = cfg;  // wall positions as saved
  if (H.vib) RC_TRY(lbmdem_set_vibration(h, 1));   // (the clock and the walls go on from cfg)
  h->force_mode = H.force_mode;
  h->L.lid6 = H.lid6;
  h->diag_always = H.diag_always != 0;
  if (H.has_carry) {  // the "previous contact" carries continue across the restart (no records yet: ct.carry stands)
    if (hipMemcpy(h->ct.carry, H.carry, sizeof H.carry, hipMemcpyHostToDevice) != hipSuccess)
      return fail(LBMDEM_EHIP, "checkpoint: carries not restored");
  }
  h->nbsteps = H.nbsteps;
  h->verlet_ok = H.verlet_ok != 0;
  h->verlet_tracks_positions = h->verlet_ok;
  // (the positions the list was built from, V.xreb / V.yreb, are not in the file: until the next rebuild the rasterisers
  // treat the list as outrun -- clear + repaint with atomics, never the list-based plain stores or the update in place)
  *h->moved_host = h->list_generation;
  if (h->verlet_ok) {  // the entry -> grain map is derived from the offsets
    launch_fill_own(h->V, n, h->stream);
    launch_tile_halo(h->V, n, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(LBMDEM_EHIP, "k_fill_own failed");
  }
  guard.h = nullptr;
  *out = h;
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

int lbmdem_checkpoint_digest(const void* bytes, size_t n, unsigned long long* out2) {
  if ((!bytes && n > 0) || !out2) return fail(LBMDEM_EINVAL, "null argument");
  u64 acc[2] = {0, 0};
  digest_add(bytes, n, 0, acc);
  out2[0] = acc[0]; out2[1] = acc[1];
  return LBMDEM_OK;
}

int lbmdem_checkpoint_verify(const char* path, int* has_digest) try {
  SP_UNAVAILABLE("checkpointing");
  if (!path || !has_digest) return fail(LBMDEM_EINVAL, "null argument");
  return verify_file(path, has_digest, false);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_checkpoint_every(lbmdem_handle* h, long every_substeps, const char* path) {
  SP_UNAVAILABLE("checkpointing");
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (every_substeps < 0) return fail(LBMDEM_EINVAL, "lbmdem_set_checkpoint_every: the cadence must be >= 0, not %ld", every_substeps);
  if (every_substeps > 0) {
    RC_TRY(whole_handle(h, "lbmdem_set_checkpoint_every", "there every rank saves its own file with lbmdem_checkpoint_save"));
    if (!path || !*path || strlen(path) >= sizeof h->ckpt_path) return fail(LBMDEM_EINVAL, "lbmdem_set_checkpoint_every: no path, or one that is too long");
    strcpy(h->ckpt_path, path);
  }
  h->ckpt_every = every_substeps;
  return LBMDEM_OK;
}

// the cadence's save without slots (lbmdem_run_scene): lbmdem_checkpoint_save's file, by way of `<path>.tmp` and rename
int lbmdem_ckpt_save_replacing(lbmdem_handle* h, const char* path) {
  char tmp[sizeof h->ckpt_path + 8];
  snprintf(tmp, sizeof tmp, "%s.tmp", path);
  const int rc = lbmdem_checkpoint_save(h, tmp);
  if (rc != LBMDEM_OK) { (void)remove(tmp); return rc; }
  if (rename(tmp, path) != 0) {
    const int err = errno;
    (void)remove(tmp);
    return fail(LBMDEM_EINVAL, "renaming '%s' onto '%s' failed: %s", tmp, path, strerror(err));
  }
  return LBMDEM_OK;
}

}  // extern "C"
#pragma GCC visibility pop
