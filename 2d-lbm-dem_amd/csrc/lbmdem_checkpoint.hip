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
// A file with an extension (lbmdem_set_checkpoint_contents: "LBMXTRA1", CkptExtra and its five sections behind f) ends in the
// trailer "LBMCKSM2" instead: the same, always CKSM2_SECTIONS entries -- the ten, the extension header ("extras"), the five
// sections of the optional state, those the file does not carry with length and digests 0. Both trailers have a fixed size, so
// either is found at the very end of a complete file.
typedef unsigned long long u64;
constexpr int CKSM_SECTIONS = 1 + CKPT_DEV_SECTIONS;
constexpr int CKSM2_SECTIONS = CKSM_SECTIONS + 1 + CKPT_XTRA_SECTIONS;
constexpr int CKSM_EXTRAS = CKSM_SECTIONS;   // the extension header's entry
static const char* const CKSM_NAMES[CKSM2_SECTIONS] = {"header", "r", "kin", "fhf", "gp", "offsets", "nbr", "wallflags", "obst", "f",
                                                       "extras", "tracers", "scalar_g", "scalar_was", "mean_cnt", "mean_S"};
struct CksmEntry { u64 bytes, s1, s2; };
struct CksmTrailer {    // "LBMCKSM1"
  char magic[8];
  int nsections, pad;
  CksmEntry e[CKSM_SECTIONS];
};
struct CksmTrailer2 {   // "LBMCKSM2"
  char magic[8];
  int nsections, pad;
  CksmEntry e[CKSM2_SECTIONS];
};
static_assert(sizeof(CksmTrailer) == 16 + 24 * CKSM_SECTIONS && sizeof(CksmTrailer2) == 16 + 24 * CKSM2_SECTIONS, "the trailers have no padding");

// ---- the extension ("LBMXTRA1", CkptExtra: lbmdem_handle.h) -----------------------------------------------------------------
constexpr int MEAN_BIT_PLANES[5] = {2, 3, 2, 2, 2};   // planes of doubles per bit of a window's mask (lbm_mean.hip's table)
static int mean_planes_of(int mask) {
  int c = 0;
  for (int b = 0; b < 5; ++b) c += ((mask >> b) & 1) ? MEAN_BIT_PLANES[b] : 0;
  return c;
}
// the lengths of the five sections an extension header announces
static void extra_lengths(const CkptExtra& X, u64 len[CKPT_XTRA_SECTIONS]) {
  const u64 plane = (u64)X.plane;
  len[0] = (X.mask & LBMDEM_CKPT_TRACERS) ? 16 * (u64)X.tr_n : 0;
  len[1] = (X.mask & LBMDEM_CKPT_SCALAR) ? 40 * plane : 0;
  len[2] = (X.mask & LBMDEM_CKPT_SCALAR) ? plane : 0;
  len[3] = (X.mask & LBMDEM_CKPT_MEAN) ? 8 * plane : 0;
  len[4] = (X.mask & LBMDEM_CKPT_MEAN) ? 8 * (u64)X.mn_nsel * plane : 0;
}
// Nothing of an extension header is trusted: every number is checked here before a length is formed or anything allocated
// from it. `plane`: lx * sy by the file's own header. null: plausible, else what is wrong with it.
static const char* extra_implausible(const CkptExtra& X, long plane) {
  if (X.mask <= 0 || (X.mask & ~LBMDEM_CKPT_ALL) || X.pad0 || X.pad1 || X.pad2 || X.pad3) return "a bad mask";
  if (X.plane != plane) return "another lattice";
  if (X.mask & LBMDEM_CKPT_TRACERS) {
    if (X.tr_n < 1 || X.tr_n > TRACER_MAX) return "a tracer count out of range";
    if ((X.tr_automatic != 0 && X.tr_automatic != 1) || X.tr_advances < 0 || X.tr_hook < 0 || X.tr_hook > X.tr_advances) return "bad tracer counters";
  } else if (X.tr_n || X.tr_automatic || X.tr_advances || X.tr_hook) return "tracer values without tracers";
  if (X.mask & LBMDEM_CKPT_SCALAR) {
    if (!(X.sc_tau > 0.5) || !isfinite(X.sc_tau)) return "a relaxation time that is not finite and larger than 0.5";
    if ((X.sc_automatic != 0 && X.sc_automatic != 1) || X.sc_steps < 0 || X.sc_hook < 0 || X.sc_hook > X.sc_steps) return "bad scalar counters";
  } else if (X.sc_tau != 0. || X.sc_automatic || X.sc_steps || X.sc_hook) return "scalar values without a scalar";
  if (X.mask & LBMDEM_CKPT_MEAN) {
    if (X.mn_mask <= 0 || (X.mn_mask & ~LBMDEM_MEAN_ALL)) return "a window mask out of range";
    if (X.mn_nsel != mean_planes_of(X.mn_mask)) return "a plane count that is not its window mask's";
    if (X.mn_every < 0 || X.mn_samples < 0 || X.mn_hook < 0) return "negative window counters";
  } else if (X.mn_mask || X.mn_every || X.mn_nsel || X.mn_samples || X.mn_hook) return "window values without a window";
  return nullptr;
}

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
// has a trailer only if one begins right behind the sections its header -- and its extension header, where it has one --
// announces: cut short, then. `lenient` (lbmdem_checkpoint_load's use): a file WITHOUT a trailer whose header cannot be read, or
// that is shorter than its header or extension claims, passes -- the loader's own checks and messages follow, as before.
static int verify_file(const char* path, int* has_digest, bool lenient) {
  *has_digest = 0;
  FILE* fp = fopen(path, "rb");
  if (!fp) return lenient ? LBMDEM_OK : fail(LBMDEM_EINVAL, "cannot open checkpoint '%s'", path);
  FileCloser closer{fp};
  struct stat stt{};
  if (fstat(fileno(fp), &stt) != 0) return lenient ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s': cannot take its size", path);
  const u64 size = (u64)stt.st_size;
  CkptHeader H;
  CksmTrailer2 T;   // (either trailer: the first one's entries are the first ten of the second's)
  memset(&T, 0, sizeof T);
  size_t tsize = 0;   // the trailer found at the end: 0 = none
  {
    CksmTrailer T1;
    if (size >= sizeof H + sizeof T1 && fseeko(fp, (off_t)(size - sizeof T1), SEEK_SET) == 0 && rd(fp, &T1, sizeof T1) &&
        memcmp(T1.magic, "LBMCKSM1", 8) == 0) {
      tsize = sizeof T1;
      memcpy(&T, &T1, sizeof T1);
    } else if (size >= sizeof H + sizeof T && fseeko(fp, (off_t)(size - sizeof T), SEEK_SET) == 0 && rd(fp, &T, sizeof T) &&
               memcmp(T.magic, "LBMCKSM2", 8) == 0) {
      tsize = sizeof T;
    }
  }
  const bool at_end = tsize != 0, two = tsize == sizeof T;
  if (fseeko(fp, 0, SEEK_SET) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot rewind", path);
  const bool have_header = rd(fp, &H, sizeof H);
  if (at_end) {
    *has_digest = 1;
    u64 acc[2] = {0, 0};
    digest_add(&H, sizeof H, 0, acc);
    if (T.nsections != (two ? CKSM2_SECTIONS : CKSM_SECTIONS) || T.pad != 0 || T.e[0].bytes != sizeof H)
      return fail(LBMDEM_EINVAL, "checkpoint '%s': its digest trailer is malformed", path);
    if (!have_header || acc[0] != T.e[0].s1 || acc[1] != T.e[0].s2)
      return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'header' does not match its digest (the file is torn or corrupted)", path);
  }
  if (!have_header || memcmp(H.magic, "LBMDEMC5", 8) != 0 || H.layout != CKPT_LAYOUT || !header_plausible(H))
    return lenient && !at_end ? LBMDEM_OK : fail(LBMDEM_EINVAL, "'%s' is not a checkpoint of this library version", path);
  u64 len[CKSM2_SECTIONS], fixed = 0;
  memset(len, 0, sizeof len);
  section_lengths(H, len);
  for (int s = 0; s < CKSM_SECTIONS; ++s) fixed += len[s];
  // the extension, where the file has one: right behind f, never in a strip's file
  CkptExtra X;
  memset(&X, 0, sizeof X);
  bool have_extra = false;
  if (H.has_dist == 0 && size > fixed) {
    const u64 rest = size - fixed;
    const size_t k = rest < sizeof X ? (size_t)rest : sizeof X;
    if (fseeko(fp, (off_t)fixed, SEEK_SET) != 0 || !rd(fp, &X, k)) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot read behind its sections", path);
    // (a file cut within the three letters both magics begin with is taken for one cut inside its trailer, as ever)
    if (memcmp(X.magic, "LBMXTRA1", k < 8 ? k : 8) == 0 && !(k < 8 && memcmp(X.magic, "LBMCKSM1", k) == 0)) {
      if (k < sizeof X)
        return lenient && !at_end ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s': its extension header is cut short (%llu of %zu bytes)", path, rest, sizeof X);
      have_extra = true;
    }
  }
  if (two && !have_extra) return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'extras' is missing behind section 'f' (the file is torn or corrupted)", path);
  if (have_extra) {
    if (at_end && two) {   // the extension header against its digest before anything is taken from it
      u64 acc[2] = {0, 0};
      digest_add(&X, sizeof X, 0, acc);
      if (T.e[CKSM_EXTRAS].bytes != sizeof X || acc[0] != T.e[CKSM_EXTRAS].s1 || acc[1] != T.e[CKSM_EXTRAS].s2)
        return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'extras' does not match its digest (the file is torn or corrupted)", path);
    }
    if (const char* why = extra_implausible(X, H.plane))
      return lenient && !at_end ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s': section 'extras' holds %s", path, why);
    len[CKSM_EXTRAS] = sizeof X;
    extra_lengths(X, len + CKSM_EXTRAS + 1);
    for (int s = CKSM_EXTRAS; s < CKSM2_SECTIONS; ++s) fixed += len[s];
  }
  const int nsec = have_extra ? CKSM2_SECTIONS : CKSM_SECTIONS;
  if (!at_end) {
    if (size < fixed) return lenient ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its header claims (%llu of at least %llu bytes)", path, size, fixed);
    const u64 rest = size - fixed;
    char head[8];
    const size_t k = rest < 8 ? (size_t)rest : 8;
    if (k == 0) return LBMDEM_OK;
    if (fseeko(fp, (off_t)fixed, SEEK_SET) != 0 || !rd(fp, head, k)) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot read behind its sections", path);
    if (memcmp(head, have_extra ? "LBMCKSM2" : "LBMCKSM1", k) != 0) return LBMDEM_OK;   // (e.g. the strips' "LBMDIST1" section)
    *has_digest = 1;
    return fail(LBMDEM_EINVAL, "checkpoint '%s': its digest trailer is cut short (%llu of %zu bytes)", path, rest,
                have_extra ? sizeof(CksmTrailer2) : sizeof(CksmTrailer));
  }
  if (two != have_extra)
    return fail(LBMDEM_EINVAL, "checkpoint '%s': an extension behind section 'f' that its digest trailer does not cover", path);
  if (fixed + tsize != size)
    return fail(LBMDEM_EINVAL, "checkpoint '%s': %llu bytes by its header and digest trailer, %llu in the file", path, fixed + (u64)tsize, size);
  if (fseeko(fp, (off_t)sizeof H, SEEK_SET) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot seek", path);
  std::vector<unsigned char> buf((size_t)1 << 22);
  for (int s = 1; s < nsec; ++s) {
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

// ---- what a save adds to the file: the optional state lbmdem_set_checkpoint_contents selects, where the handle has it ----------
CkptLayout lbmdem_ckpt_extra(const lbmdem_handle* h, CkptExtra* X) {
  memset(X, 0, sizeof *X);
  const TracerState& T = h->tracers;
  const ScalarState& S = h->scalar;
  const MeanState& M = h->mean;
  const int want = h->dist ? 0 : h->ckpt_contents;   // (a strip's file has its own trailing section and no extension)
  if ((want & LBMDEM_CKPT_TRACERS) && T.n > 0) {
    X->mask |= LBMDEM_CKPT_TRACERS;
    X->tr_n = T.n; X->tr_automatic = T.automatic ? 1 : 0; X->tr_advances = T.advances; X->tr_hook = T.hook;
  }
  if ((want & LBMDEM_CKPT_SCALAR) && S.on) {
    X->mask |= LBMDEM_CKPT_SCALAR;
    X->sc_tau = S.tau; X->sc_automatic = S.automatic ? 1 : 0; X->sc_steps = S.steps; X->sc_hook = S.hook;
  }
  if ((want & LBMDEM_CKPT_MEAN) && M.on) {
    X->mask |= LBMDEM_CKPT_MEAN;
    X->mn_mask = M.mask; X->mn_every = M.every; X->mn_nsel = M.nsel; X->mn_samples = M.samples; X->mn_hook = M.hook;
  }
  if (!X->mask) return ckpt_layout(h->n, h->V.cap, h->L.plane);
  memcpy(X->magic, "LBMXTRA1", 8);
  X->plane = (long)h->L.lx * h->L.sy;
  u64 len[CKPT_XTRA_SECTIONS];
  extra_lengths(*X, len);
  size_t xb[CKPT_XTRA_SECTIONS];
  for (int s = 0; s < CKPT_XTRA_SECTIONS; ++s) xb[s] = (size_t)len[s];
  return ckpt_layout(h->n, h->V.cap, h->L.plane, xb);
}

#ifndef LBMDEM_SINGLE_PRECISION
// ---- checkpoints in the background: the two ends of a slot's way (the middle is lbmdem_output.hip's) --------------------------
void lbmdem_ckpt_frame_job(const lbmdem_handle* h, const CkptLayout& Y, unsigned char* staging, CkptFrameJob* J) {
  // (a section of length 0 is never read: its source may be anything)
  const void* src[CKPT_ALL_SECTIONS] = {h->r, h->kin[h->kcur].x1, h->fhf, h->gp, h->verlet_ok ? h->V.offsets : nullptr,
                                        h->V.nbr, h->V.wallflags, h->obst[h->ocur], h->f[h->fcur],
                                        h->tracers.xy, h->scalar.g[h->scalar.cur], h->scalar.was, h->mean.cnt, h->mean.S};
  for (int s = 0; s < CKPT_ALL_SECTIONS; ++s) { J->src[s] = src[s]; J->bytes[s] = Y.bytes[s]; J->at[s] = Y.at[s]; }
  J->nnbr = h->verlet_ok ? h->V.offsets + h->n : nullptr;   // (lbmdem_checkpoint_save: zero offsets, no entries without a list)
  J->carry = h->ct.carry;
  J->staging = staging;
  J->gate = h->L.gate;
}

int lbmdem_ckpt_write_slot(const AsyncSlot* S, char* msg, size_t msglen) {
  const CkptLayout* Y = &S->ckpt_layout;
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
  const CkptExtra& X = C.xtra;
  const bool extra = X.mask != 0;   // then "LBMCKSM2" with all its entries, else the trailer of every file so far
  CksmTrailer2 T;
  memset(&T, 0, sizeof T);
  memcpy(T.magic, extra ? "LBMCKSM2" : "LBMCKSM1", 8);
  T.nsections = extra ? CKSM2_SECTIONS : CKSM_SECTIONS;
  const size_t tsize = extra ? sizeof(CksmTrailer2) : sizeof(CksmTrailer);
  {
    u64 acc[2] = {0, 0};
    digest_add(&H, sizeof H, 0, acc);
    T.e[0] = CksmEntry{sizeof H, acc[0], acc[1]};
  }
  for (int s = 0; s < CKPT_DEV_SECTIONS; ++s) {
    const u64 bytes = s == CKPT_NBR ? 4 * (u64)H.nnbr : Y->bytes[s];
    T.e[1 + s] = CksmEntry{bytes, words[4 + 2 * s], words[5 + 2 * s]};
  }
  if (extra) {
    u64 acc[2] = {0, 0};
    digest_add(&X, sizeof X, 0, acc);
    T.e[CKSM_EXTRAS] = CksmEntry{sizeof X, acc[0], acc[1]};
    for (int s = CKPT_DEV_SECTIONS; s < CKPT_ALL_SECTIONS; ++s)   // (a section of length 0 has added nothing: digests 0)
      T.e[CKSM_EXTRAS + 1 + s - CKPT_DEV_SECTIONS] = CksmEntry{Y->bytes[s], words[4 + 2 * s], words[5 + 2 * s]};
  }
  char tmp[sizeof S->path + 8];
  snprintf(tmp, sizeof tmp, "%s.tmp", S->path);
  FILE* fp = fopen(tmp, "wb");
  if (!fp) { snprintf(msg, msglen, "cannot open '%s' for writing: %s", tmp, strerror(errno)); return LBMDEM_EINVAL; }
  bool ok = wr(fp, &H, sizeof H);
  for (int s = 0; s < CKPT_DEV_SECTIONS && ok; ++s) ok = wr(fp, image + Y->at[s], (size_t)T.e[1 + s].bytes);   // exact lengths
  if (extra && ok) ok = wr(fp, &X, sizeof X);
  for (int s = CKPT_DEV_SECTIONS; s < CKPT_ALL_SECTIONS && extra && ok; ++s) ok = wr(fp, image + Y->at[s], Y->bytes[s]);
  if (ok) ok = wr(fp, &T, tsize);
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
  CkptExtra X;   // the handle has settled and its stream is idle: the counters are those of the state on the device
  (void)lbmdem_ckpt_extra(h, &X);
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
  if (X.mask && ok) {   // the extension: its header, then the five sections, plane by plane (bounded host staging)
    const size_t plane = (size_t)X.plane;
    ok = wr(fp, &X, sizeof X);
    if (X.mask & LBMDEM_CKPT_TRACERS) dump(h->tracers.xy, 16 * (size_t)X.tr_n);
    if (X.mask & LBMDEM_CKPT_SCALAR) {
      for (int k = 0; k < 5; ++k) dump(h->scalar.g[h->scalar.cur] + k * plane, sizeof(double) * plane);
      dump(h->scalar.was, plane);
    }
    if (X.mask & LBMDEM_CKPT_MEAN) {
      for (int k = 0; k < 2; ++k) dump(h->mean.cnt + k * plane, sizeof(unsigned) * plane);
      for (int k = 0; k < X.mn_nsel; ++k) dump(h->mean.S + k * plane, sizeof(double) * plane);
    }
  }
  ok = (fclose(fp) == 0) && ok;
  if (!ok) return fail(LBMDEM_EHIP, "writing checkpoint '%s' failed", path);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

// The extension of the file, where it has one: `fp` stands behind f. Everything is checked before it is used: the header's
// numbers, the sections' lengths against the file, the positions (lbmdem_tracer_set's own test), the bytes of `was`. The states
// are then set up the way their setters do it -- lbmdem_tracer_set, lbmdem_scalar_set (which forms omega = 1. / tau),
// lbmdem_mean_begin -- and filled with the file's sections and counters.
static int load_extra(const char* path, FILE* fp, lbmdem_handle* h) {
  const off_t at0 = ftello(fp);
  struct stat stt{};
  if (at0 < 0 || fstat(fileno(fp), &stt) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot take its size", path);
  const u64 rest = (u64)stt.st_size - (u64)at0;
  CkptExtra X;
  if (rest < 8 || !rd(fp, X.magic, 8) || memcmp(X.magic, "LBMXTRA1", 8) != 0) return LBMDEM_OK;   // a plain file (or its trailer)
  if (rest < sizeof X || !rd(fp, reinterpret_cast<char*>(&X) + 8, sizeof X - 8))
    return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension header is cut short", path);
  const LatticeView& L = h->L;
  const size_t plane = (size_t)L.lx * L.sy;
  if (const char* why = extra_implausible(X, (long)plane)) return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension holds %s", path, why);
  u64 len[CKPT_XTRA_SECTIONS], need = sizeof X;
  extra_lengths(X, len);
  for (int s = 0; s < CKPT_XTRA_SECTIONS; ++s) need += len[s];
  if (rest < need)
    return fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its extension claims (%llu of at least %llu bytes behind section 'f')", path, rest, need);
  bool ok = true;
  std::vector<char> buf;
  auto fill = [&](void* dev, size_t bytes) {   // (lbmdem_checkpoint_load's: one piece of bounded size at a time)
    if (!ok || bytes == 0) return;
    buf.resize(bytes);
    ok = rd(fp, buf.data(), bytes) && hipMemcpy(dev, buf.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (X.mask & LBMDEM_CKPT_TRACERS) {
    std::vector<double> xy(2 * (size_t)X.tr_n);   // (16 tr_n bytes are in the file)
    if (!rd(fp, xy.data(), sizeof(double) * xy.size())) return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'tracers' cannot be read", path);
    RC_TRY(lbmdem_tracer_set(h, X.tr_n, xy.data(), X.tr_automatic));   // refuses a position outside the lattice, NaN included
    h->tracers.advances = X.tr_advances;
    h->tracers.hook = X.tr_hook;
  }
  if (X.mask & LBMDEM_CKPT_SCALAR) {
    {   // `was` lies behind the populations: looked at first, nothing is allocated for a file whose flags are not flags
      const off_t at_g = ftello(fp);
      std::vector<unsigned char> was(plane);
      if (at_g < 0 || fseeko(fp, at_g + (off_t)len[1], SEEK_SET) != 0 || !rd(fp, was.data(), plane) || fseeko(fp, at_g, SEEK_SET) != 0)
        return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'scalar_was' cannot be read", path);
      for (size_t k = 0; k < plane; ++k)
        if (was[k] > 1) return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'scalar_was' holds the byte %d at %zu (0 or 1 expected)", path, was[k], k);
    }
    {
      const std::vector<double> zero((size_t)L.lx * L.ly, 0.);
      RC_TRY(lbmdem_scalar_set(h, zero.data(), X.sc_tau, X.sc_automatic));
    }
    ScalarState& S = h->scalar;
    for (int k = 0; k < 5; ++k) fill(S.g[S.cur] + k * plane, sizeof(double) * plane);
    fill(S.was, plane);
    S.steps = X.sc_steps;
    S.hook = X.sc_hook;
  }
  if (X.mask & LBMDEM_CKPT_MEAN) {
    RC_TRY(lbmdem_mean_begin(h, X.mn_mask, X.mn_every));
    MeanState& M = h->mean;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(LBMDEM_EHIP, "checkpoint: the window could not be set up");   // (its zeroing)
    for (int k = 0; k < 2; ++k) fill(M.cnt + k * plane, sizeof(unsigned) * plane);
    for (int k = 0; k < M.nsel; ++k) fill(M.S + k * plane, sizeof(double) * plane);
    M.samples = X.mn_samples;
    M.hook = X.mn_hook;
    M.resumed = true;
  }
  if (!ok) return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension cannot be read or copied to the device", path);
  return LBMDEM_OK;
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
  if (!H.has_dist) RC_TRY(load_extra(path, fp, h));   // (a refusal leaves through the guard: the file is refused as a whole)
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

int lbmdem_set_checkpoint_contents(lbmdem_handle* h, int mask) {
  SP_UNAVAILABLE("checkpointing");
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (mask < 0 || (mask & ~LBMDEM_CKPT_ALL)) return fail(LBMDEM_EINVAL, "lbmdem_set_checkpoint_contents: bad mask %d", mask);
  if (mask) RC_TRY(whole_handle(h, "lbmdem_set_checkpoint_contents", "there a checkpoint holds a rank's strip and nothing else"));
  h->ckpt_contents = mask;
  return LBMDEM_OK;
}

int lbmdem_checkpoint_contents(const char* path, long* out5) {
  SP_UNAVAILABLE("checkpointing");
  if (!path || !out5) return fail(LBMDEM_EINVAL, "null argument");
  for (int k = 0; k < 5; ++k) out5[k] = 0;
  FILE* fp = fopen(path, "rb");
  if (!fp) return fail(LBMDEM_EINVAL, "cannot open checkpoint '%s'", path);
  FileCloser closer{fp};
  struct stat stt{};
  CkptHeader H;
  if (fstat(fileno(fp), &stt) != 0 || !rd(fp, &H, sizeof H) || memcmp(H.magic, "LBMDEMC5", 8) != 0 || H.layout != CKPT_LAYOUT ||
      !header_plausible(H))
    return fail(LBMDEM_EINVAL, "'%s' is not a checkpoint of this library version", path);
  u64 len[CKSM_SECTIONS], fixed = 0;
  section_lengths(H, len);
  for (int s = 0; s < CKSM_SECTIONS; ++s) fixed += len[s];
  const u64 size = (u64)stt.st_size;
  if (size < fixed) return fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its header claims (%llu of at least %llu bytes)", path, size, fixed);
  CkptExtra X;
  if (H.has_dist || size - fixed < 8 || fseeko(fp, (off_t)fixed, SEEK_SET) != 0 || !rd(fp, X.magic, 8) || memcmp(X.magic, "LBMXTRA1", 8) != 0)
    return LBMDEM_OK;   // a plain file
  if (size - fixed < sizeof X || !rd(fp, reinterpret_cast<char*>(&X) + 8, sizeof X - 8))
    return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension header is cut short", path);
  if (const char* why = extra_implausible(X, H.plane)) return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension holds %s", path, why);
  out5[0] = X.mask; out5[1] = X.tr_n; out5[2] = X.sc_steps; out5[3] = X.mn_mask; out5[4] = X.mn_samples;
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
