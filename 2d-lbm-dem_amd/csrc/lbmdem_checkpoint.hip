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
// a trailer's entries are the two headers and CKPT_TABLE's sections: "header", the nine, "extras", the five
static int cksm_entry(int s) { return s < CKPT_DEV_SECTIONS ? 1 + s : 2 + s; }
static const char* cksm_name(int e) { return e == 0 ? "header" : e == CKSM_EXTRAS ? "extras" : CKPT_TABLE[e < CKSM_EXTRAS ? e - 1 : e - 2].name; }
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

// the numbers of a file's two headers that its sections' lengths follow from (X null: a file without an extension)
static CkptDims ckpt_dims(const CkptHeader& H, const CkptExtra* X) {
  return CkptDims{(size_t)H.cfg.nbgrains, (size_t)H.nnbr, (size_t)H.plane, X ? (size_t)X->tr_n : 0, X ? (size_t)X->mn_nsel : 0, X ? X->mask : 0};
}
// the lengths of a file's sections as its trailer lists them (X null: the last six are 0) -> their sum
static u64 section_lengths(const CkptHeader& H, const CkptExtra* X, u64 len[CKSM2_SECTIONS]) {
  const CkptDims D = ckpt_dims(H, X);
  len[0] = sizeof H;
  len[CKSM_EXTRAS] = X ? sizeof *X : 0;
  u64 sum = len[0] + len[CKSM_EXTRAS];
  for (int s = 0; s < CKPT_ALL_SECTIONS; ++s) sum += len[cksm_entry(s)] = ckpt_section_bytes(s, D);
  return sum;
}

// The extension behind f (never in a strip's file): `at` is the offset behind f, `size` the file's, `plane` lx * sy by the file's
// header. XTRA_NONE: what follows f, if anything, is no extension (a trailer, also one cut within the three letters both magics
// begin with). XTRA_OK: *X, checked. XTRA_REFUSED: *X holds *why (extra_implausible), or with *why null is cut short or unreadable.
enum { XTRA_NONE, XTRA_OK, XTRA_REFUSED };
static int read_extension(FILE* fp, u64 at, u64 size, long plane, CkptExtra* X, const char** why) {
  memset(X, 0, sizeof *X);
  *why = nullptr;
  if (size <= at) return XTRA_NONE;
  const size_t k = size - at < sizeof *X ? (size_t)(size - at) : sizeof *X;
  if (fseeko(fp, (off_t)at, SEEK_SET) != 0 || !rd(fp, X, k)) return XTRA_REFUSED;
  if (memcmp(X->magic, "LBMXTRA1", k < 8 ? k : 8) != 0 || (k < 8 && memcmp(X->magic, "LBMCKSM1", k) == 0)) return XTRA_NONE;
  if (k < sizeof *X) return XTRA_REFUSED;
  *why = extra_implausible(*X, plane);
  return *why ? XTRA_REFUSED : XTRA_OK;
}
// the refusal's message of the paths that read without a trailer (the loader, lbmdem_checkpoint_contents)
static int extension_refused(const char* path, const char* why) {
  if (!why) return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension header is cut short", path);
  return fail(LBMDEM_EINVAL, "checkpoint '%s': its extension holds %s", path, why);
}

// CkptHeader from the host's side as it stood, the pair list's length and the three carries; has_dist stays 0
static void ckpt_header(CkptHeader* H, const CkptShot& C, int nnbr, const void* carry3) {
  memset(H, 0, sizeof *H);
  memcpy(H->magic, "LBMDEMC5", 8);
  H->lid6 = C.lid6;
  H->layout = CKPT_LAYOUT; H->force_mode = C.force_mode; H->diag_always = C.diag_always;
  H->has_carry = 1;
  memcpy(H->carry, carry3, sizeof H->carry);
  H->cfg = C.cfg; H->nbsteps = C.nbsteps; H->verlet_ok = C.verlet_ok; H->nnbr = nnbr; H->plane = C.plane;
  H->vib = C.vib;
}

// where a section's bytes lie on a handle (a section of length 0 is never read: its place may be anything)
static void* ckpt_where(const lbmdem_handle* h, int s) {
  switch (s) {
    case CKPT_R: return h->r;                 case CKPT_KIN: return h->kin[h->kcur].x1;
    case CKPT_FHF: return h->fhf;             case CKPT_GP: return h->gp;
    case CKPT_OFFSETS: return h->V.offsets;   case CKPT_NBR: return h->V.nbr;   // (zero offsets in the file without a pair list)
    case CKPT_WALLFLAGS: return h->V.wallflags;
    case CKPT_OBST: return h->obst[h->ocur];  case CKPT_F: return h->f[h->fcur];
    case CKPT_TRACERS: return h->tracers.xy;
    case CKPT_SCALAR_G: return h->scalar.g[h->scalar.cur];   case CKPT_SCALAR_WAS: return h->scalar.was;
    case CKPT_MEAN_CNT: return h->mean.cnt;   default: return h->mean.S;
  }
}
// `bytes` between the device and the file in pieces of at most `piece`: bounded host staging
static bool ckpt_copy(FILE* fp, void* dev, size_t bytes, size_t piece, bool to_file) {
  std::vector<char> buf(bytes < piece ? bytes : piece);
  for (size_t done = 0; done < bytes; done += buf.size()) {
    const size_t k = bytes - done < buf.size() ? bytes - done : buf.size();
    char* at = static_cast<char*>(dev) + done;
    if (to_file ? hipMemcpy(buf.data(), at, k, hipMemcpyDeviceToHost) != hipSuccess || !wr(fp, buf.data(), k)
                : !rd(fp, buf.data(), k) || hipMemcpy(at, buf.data(), k, hipMemcpyHostToDevice) != hipSuccess) return false;
  }
  return true;
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
  u64 len[CKSM2_SECTIONS];
  u64 fixed = section_lengths(H, nullptr, len);
  // the extension, where the file has one: right behind f, never in a strip's file
  CkptExtra X;
  const char* why = nullptr;
  const int xr = H.has_dist == 0 ? read_extension(fp, fixed, size, H.plane, &X, &why) : XTRA_NONE;
  if (xr == XTRA_REFUSED && !why)
    return lenient && !at_end ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s': its extension header is cut short (%llu of %zu bytes)", path, size - fixed, sizeof X);
  const bool have_extra = xr != XTRA_NONE;
  if (two && !have_extra) return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'extras' is missing behind section 'f' (the file is torn or corrupted)", path);
  if (have_extra) {
    if (at_end && two) {   // the extension header against its digest before anything is taken from it
      u64 acc[2] = {0, 0};
      digest_add(&X, sizeof X, 0, acc);
      if (T.e[CKSM_EXTRAS].bytes != sizeof X || acc[0] != T.e[CKSM_EXTRAS].s1 || acc[1] != T.e[CKSM_EXTRAS].s2)
        return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'extras' does not match its digest (the file is torn or corrupted)", path);
    }
    if (why) return lenient && !at_end ? LBMDEM_OK : fail(LBMDEM_EINVAL, "checkpoint '%s': section 'extras' holds %s", path, why);
    fixed = section_lengths(H, &X, len);
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
                  cksm_name(s), len[s], T.e[s].bytes);
    u64 acc[2] = {0, 0};
    for (u64 done = 0; done < len[s];) {
      const size_t piece = len[s] - done < buf.size() ? (size_t)(len[s] - done) : buf.size();
      if (!rd(fp, buf.data(), piece)) return fail(LBMDEM_EINVAL, "checkpoint '%s': section '%s' cannot be read", path, cksm_name(s));
      digest_add(buf.data(), piece, done / 8, acc);
      done += piece;
    }
    if (acc[0] != T.e[s].s1 || acc[1] != T.e[s].s2)
      return fail(LBMDEM_EINVAL, "checkpoint '%s': section '%s' does not match its digest (the file is torn or corrupted)", path, cksm_name(s));
  }
  return LBMDEM_OK;
}
}  // namespace

// ---- what a save adds to the file: the optional state lbmdem_set_checkpoint_contents selects, where the handle has it ----------
CkptLayout lbmdem_ckpt_shot(const lbmdem_handle* h, CkptShot* C) {
  C->cfg = h->cfg; C->nbsteps = h->nbsteps; C->plane = h->L.plane; C->lid6 = h->L.lid6;
  C->force_mode = h->force_mode; C->diag_always = h->diag_always ? 1 : 0; C->verlet_ok = h->verlet_ok ? 1 : 0; C->vib = h->vib ? 1 : 0;
  CkptExtra* X = &C->xtra;
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
  if (X->mask) {
    memcpy(X->magic, "LBMXTRA1", 8);
    X->plane = (long)h->L.lx * h->L.sy;
  }
  // (a slot holds CKPT_NBR at the list's capacity: its length is known only on the device when the slot is laid out)
  return ckpt_layout(CkptDims{(size_t)h->n, (size_t)h->V.cap, (size_t)h->L.plane, (size_t)X->tr_n, (size_t)X->mn_nsel, X->mask});
}

#ifndef LBMDEM_SINGLE_PRECISION
// ---- checkpoints in the background: the two ends of a slot's way (the middle is lbmdem_output.hip's) --------------------------
void lbmdem_ckpt_frame_job(const lbmdem_handle* h, const CkptLayout& Y, unsigned char* staging, CkptFrameJob* J) {
  for (int s = 0; s < CKPT_ALL_SECTIONS; ++s) { J->src[s] = ckpt_where(h, s); J->bytes[s] = Y.bytes[s]; J->at[s] = Y.at[s]; }
  if (!h->verlet_ok) J->src[CKPT_OFFSETS] = nullptr;        // without a pair list: zero offsets, no entries (as lbmdem_checkpoint_save)
  J->nnbr = h->verlet_ok ? h->V.offsets + h->n : nullptr;
  J->carry = h->ct.carry;
  J->staging = staging;
  J->gate = h->L.gate;
}

int lbmdem_ckpt_write_slot(const AsyncSlot* S, char* msg, size_t msglen) {
  const CkptLayout* Y = &S->ckpt_layout;
  const unsigned char* image = static_cast<const unsigned char*>(S->pinned);
  const u64* words = reinterpret_cast<const u64*>(image);
  CkptHeader H;
  ckpt_header(&H, S->shot, (int)words[0], words + 1);
  const CkptExtra& X = S->shot.xtra;
  const bool extra = X.mask != 0;   // then "LBMCKSM2" with all its entries, else the trailer of every file so far
  CksmTrailer2 T;
  memset(&T, 0, sizeof T);
  memcpy(T.magic, extra ? "LBMCKSM2" : "LBMCKSM1", 8);
  T.nsections = extra ? CKSM2_SECTIONS : CKSM_SECTIONS;
  const size_t tsize = extra ? sizeof(CksmTrailer2) : sizeof(CksmTrailer);
  const int nsec = extra ? CKPT_ALL_SECTIONS : CKPT_DEV_SECTIONS;
  u64 len[CKSM2_SECTIONS];   // the file's lengths: CKPT_NBR at 4 * nnbr, not at the capacity the slot holds it at
  (void)section_lengths(H, extra ? &X : nullptr, len);
  u64 acc[4] = {0, 0, 0, 0};
  digest_add(&H, sizeof H, 0, acc);
  T.e[0] = CksmEntry{sizeof H, acc[0], acc[1]};
  if (extra) digest_add(&X, sizeof X, 0, acc + 2);
  if (extra) T.e[CKSM_EXTRAS] = CksmEntry{sizeof X, acc[2], acc[3]};
  for (int s = 0; s < nsec; ++s)   // (a section of length 0 has added nothing: digests 0)
    T.e[cksm_entry(s)] = CksmEntry{len[cksm_entry(s)], words[4 + 2 * s], words[5 + 2 * s]};
  char tmp[sizeof S->path + 8];
  snprintf(tmp, sizeof tmp, "%s.tmp", S->path);
  FILE* fp = fopen(tmp, "wb");
  if (!fp) { snprintf(msg, msglen, "cannot open '%s' for writing: %s", tmp, strerror(errno)); return LBMDEM_EINVAL; }
  bool ok = wr(fp, &H, sizeof H);
  for (int s = 0; s < nsec && ok; ++s) {
    if (s == CKPT_DEV_SECTIONS) ok = wr(fp, &X, sizeof X);
    if (ok) ok = wr(fp, image + Y->at[s], (size_t)len[cksm_entry(s)]);
  }
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
  std::vector<int> off(n + 1, 0);   // (the offsets of a handle without a pair list are zeros in the file)
  if (h->verlet_ok) HIP_TRY(hipMemcpy(off.data(), h->V.offsets, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
  CkptShot C;   // the handle has settled and its stream is idle: the counters are those of the state on the device
  (void)lbmdem_ckpt_shot(h, &C);
  const CkptExtra& X = C.xtra;
  if (!h->dist && h->carry_from < h->substep_seq) {
    launch_carry_resolve(h->ct, h->carry_from, h->stream);
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  double carry[3];
  HIP_TRY(hipMemcpy(carry, h->ct.carry, sizeof carry, hipMemcpyDeviceToHost));
  CkptHeader H;
  ckpt_header(&H, C, off[n], carry);
  H.has_dist = h->dist ? 1 : 0;
  const CkptDims D = ckpt_dims(H, &X);
  const size_t piece = sizeof(double) * D.plane;   // f and the extension's sections of several planes go plane by plane
  FILE* fp = fopen(path, "wb");
  if (!fp) return fail(LBMDEM_EINVAL, "cannot open '%s' for writing", path);
  bool ok = wr(fp, &H, sizeof H);
  for (int s = 0; s < CKPT_ALL_SECTIONS && ok; ++s) {
    if (s == CKPT_DEV_SECTIONS) {   // behind f: a strip's own part, or the extension (never both), or nothing
      if (h->dist) {
        CkptDist Q;
        memset(&Q, 0, sizeof Q);
        memcpy(Q.magic, "LBMDIST1", 8);
        Q.margin = h->dist_margin; Q.cap_g = h->dd.cap_g; Q.cap_t = h->dd.cap_t; Q.cap_l = h->dd.cap_l;
        Q.poison = h->dist_poison ? 1 : 0;
        ok = wr(fp, &Q, sizeof Q) && ckpt_copy(fp, h->dd.active, n, piece, true) && ckpt_copy(fp, h->dd.fluidmask, n, piece, true) &&
             ckpt_copy(fp, h->owner, n, piece, true);
      }
      if (!X.mask) break;
      ok = wr(fp, &X, sizeof X);
    }
    const size_t bytes = ckpt_section_bytes(s, D);
    if (ok) ok = s == CKPT_OFFSETS ? wr(fp, off.data(), bytes) : ckpt_copy(fp, ckpt_where(h, s), bytes, piece, true);
  }
  ok = (fclose(fp) == 0) && ok;
  if (!ok) return fail(LBMDEM_EHIP, "writing checkpoint '%s' failed", path);
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
} catch (...) {
  return fail(LBMDEM_EINVAL, "unexpected C++ exception");
}

// section s of the file, at which `fp` stands, to its place on the handle, a plane's worth at a time; len: section_lengths
static bool fill_section(FILE* fp, lbmdem_handle* h, int s, const u64* len) {
  return ckpt_copy(fp, ckpt_where(h, s), (size_t)len[cksm_entry(s)], sizeof(double) * (size_t)h->L.plane, false);
}

// The extension of the file, where it has one: `at` is the offset behind f, `size` the file's. Everything is checked before it
// is used: the header's numbers, the sections' lengths against the file, the positions (lbmdem_tracer_set's own test), the bytes
// of `was`. The states are then set up the way their setters do it -- lbmdem_tracer_set, lbmdem_scalar_set (which forms omega =
// 1. / tau), lbmdem_mean_begin -- and filled with the file's sections and counters.
static int load_extra(const char* path, FILE* fp, u64 at, u64 size, const CkptHeader& H, lbmdem_handle* h) {
  CkptExtra X;
  const char* why = nullptr;
  const int xr = read_extension(fp, at, size, H.plane, &X, &why);
  if (xr == XTRA_NONE) return LBMDEM_OK;   // a plain file (or its trailer)
  if (xr == XTRA_REFUSED) return extension_refused(path, why);
  u64 len[CKSM2_SECTIONS];
  const u64 need = section_lengths(H, &X, len) - at, rest = size - at;
  if (rest < need)
    return fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its extension claims (%llu of at least %llu bytes behind section 'f')", path, rest, need);
  bool ok = true;
  if (X.mask & LBMDEM_CKPT_TRACERS) {
    std::vector<double> xy(2 * (size_t)X.tr_n);
    if (!rd(fp, xy.data(), (size_t)len[cksm_entry(CKPT_TRACERS)])) return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'tracers' cannot be read", path);
    RC_TRY(lbmdem_tracer_set(h, X.tr_n, xy.data(), X.tr_automatic));   // refuses a position outside the lattice, NaN included
    h->tracers.advances = X.tr_advances;
    h->tracers.hook = X.tr_hook;
  }
  if (X.mask & LBMDEM_CKPT_SCALAR) {
    {   // `was` lies behind the populations: looked at first, nothing is allocated for a file whose flags are not flags
      const off_t at_g = ftello(fp);
      std::vector<unsigned char> was((size_t)len[cksm_entry(CKPT_SCALAR_WAS)]);
      if (at_g < 0 || fseeko(fp, at_g + (off_t)len[cksm_entry(CKPT_SCALAR_G)], SEEK_SET) != 0 || !rd(fp, was.data(), was.size()) ||
          fseeko(fp, at_g, SEEK_SET) != 0)
        return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'scalar_was' cannot be read", path);
      for (size_t k = 0; k < was.size(); ++k)
        if (was[k] > 1) return fail(LBMDEM_EINVAL, "checkpoint '%s': section 'scalar_was' holds the byte %d at %zu (0 or 1 expected)", path, was[k], k);
    }
    {
      const std::vector<double> zero((size_t)h->L.lx * h->L.ly, 0.);
      RC_TRY(lbmdem_scalar_set(h, zero.data(), X.sc_tau, X.sc_automatic));
    }
    ok = fill_section(fp, h, CKPT_SCALAR_G, len) && fill_section(fp, h, CKPT_SCALAR_WAS, len);
    h->scalar.steps = X.sc_steps;
    h->scalar.hook = X.sc_hook;
  }
  if (X.mask & LBMDEM_CKPT_MEAN) {
    RC_TRY(lbmdem_mean_begin(h, X.mn_mask, X.mn_every));
    MeanState& M = h->mean;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(LBMDEM_EHIP, "checkpoint: the window could not be set up");   // (its zeroing)
    ok = ok && fill_section(fp, h, CKPT_MEAN_CNT, len) && fill_section(fp, h, CKPT_MEAN_S, len);
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
  u64 len[CKSM2_SECTIONS];
  const u64 need = section_lengths(H, nullptr, len);   // nothing is allocated from a header the file itself cannot back
  struct stat stt{};
  if (fstat(fileno(fp), &stt) != 0) return fail(LBMDEM_EINVAL, "checkpoint '%s': cannot take its size (at least %llu bytes needed)", path, need);
  if ((u64)stt.st_size < need)
    return fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its header claims (%llu of at least %llu bytes)", path, (u64)stt.st_size, need);
  std::vector<double> r(n), kin(9 * (size_t)n);
  if (!rd(fp, r.data(), (size_t)len[cksm_entry(CKPT_R)]) || !rd(fp, kin.data(), (size_t)len[cksm_entry(CKPT_KIN)])) return fail(LBMDEM_EINVAL, "checkpoint truncated");
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
  h->kcur = h->ocur = h->fcur = 0;   // where ckpt_where puts kin, obst and f
  h->obst_pending = false;
  h->chg_state[0] = h->chg_state[1] = 0;
  h->snap_ok[0] = h->snap_ok[1] = false;   // (the loaded map is not the picture lbmdem_create has just painted)
  h->geo_buf = -1;                         // (... nor do the centres of that paint describe it)
  for (int s = CKPT_KIN; s < CKPT_DEV_SECTIONS && ok; ++s) {   // (r went into lbmdem_create, which derives the rest of a grain from it)
    if (s == CKPT_KIN) {
      ok = hipMemcpy(ckpt_where(h, s), kin.data(), (size_t)len[cksm_entry(s)], hipMemcpyHostToDevice) == hipSuccess;
    } else if (s == CKPT_OFFSETS) {   // with CKPT_NBR: the pair list goes straight into kernels that index with it, checked here, on the host
      std::vector<int> off((size_t)n + 1), nb((size_t)H.nnbr);
      ok = rd(fp, off.data(), sizeof(int) * off.size()) && rd(fp, nb.data(), sizeof(int) * nb.size());
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
    } else if (s != CKPT_NBR) {
      ok = fill_section(fp, h, s, len);
    }
  }
  if (ok && H.has_dist) {   // a strip with distributed grains: masks and message capacities as the writer had them. A
    CkptDist D;             // missing or short section fails the load HERE, not later inside a collective on one rank
    const size_t piece = sizeof(double) * (size_t)H.plane;
    ok = rd(fp, &D, sizeof D) && memcmp(D.magic, "LBMDIST1", 8) == 0 && D.margin > 0 && D.cap_g > 0 && D.cap_t > 0 &&
         D.cap_l > 0 && D.cap_g <= n && D.cap_t <= n && D.cap_l <= n &&
         lbmdem_dist_enable_caps(h, D.margin, D.cap_g, D.cap_t, D.cap_l) == LBMDEM_OK &&
         ckpt_copy(fp, h->dd.active, n, piece, false) && ckpt_copy(fp, h->dd.fluidmask, n, piece, false) && ckpt_copy(fp, h->owner, n, piece, false);
    if (ok) h->dist_poison = D.poison != 0;
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
  if (!H.has_dist) RC_TRY(load_extra(path, fp, need, (u64)stt.st_size, H, h));   // (a refusal leaves through the guard: the file is refused as a whole)
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
  u64 len[CKSM2_SECTIONS];
  const u64 fixed = section_lengths(H, nullptr, len), size = (u64)stt.st_size;
  if (size < fixed) return fail(LBMDEM_EINVAL, "checkpoint '%s' is shorter than its header claims (%llu of at least %llu bytes)", path, size, fixed);
  CkptExtra X;
  const char* why = nullptr;
  const int xr = H.has_dist ? XTRA_NONE : read_extension(fp, fixed, size, H.plane, &X, &why);
  if (xr == XTRA_NONE) return LBMDEM_OK;   // a plain file
  if (xr == XTRA_REFUSED) return extension_refused(path, why);
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
