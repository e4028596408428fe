// lbmdem_handle.h -- what the translation units of the C ABI share (lbmdem_capi.hip: handle, step driver, state
// transfer; lbmdem_output.hip: the reference's file writers; lbmdem_checkpoint.hip; lbmdem_strips.hip: strip
// decomposition; lbmdem_comm.hip: the RCCL transport). Not part of the public ABI.
#pragma once

#include "../../include/lbmdem_hip.h"
#include "lbmdem_internal.h"

#include <ctype.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#define REF_PI 3.14159265358979 /* main.c:42 */
#define RHO_S 2650              /* main.c:44 */

// sets the text lbmdem_last_error() returns (thread-local) and returns `code`
int lbmdem_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail lbmdem_fail

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail(LBMDEM_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                                  \
  } while (0)
#define RC_TRY(expr) do { int rc_ = (expr); if (rc_ != LBMDEM_OK) return rc_; } while (0)

// What lbmdem_run / lbmdem_run_dem were asked for, call by call, since the stream was last known to be sound ...
struct RunLogEntry { int fluid; long n; };
// ... and the host's side of the handle as of just before a launch of k_dem_chain (everything that moves from launch to
// launch): if that launch gives up, every kernel behind it returns at once (the stop word, LatticeView::gate), the device
// holds exactly this state, and the host goes back to it and replays the log one launch per sub-step (chain_recover,
// lbmdem_capi.hip).
struct ChainSnap {
  long long seq;      // sequence number of the launch's first sub-step (what the failing kernel reports)
  long log_idx, done; // the run-log entry the launch belongs to, and the sub-steps of that call that were done before it
  int fcur, ocur, kcur, obst_reset_rows, snap_cur[2], chg_state[2], list_generation;
  bool obst_pending, snap_ok[2], diag_valid, contacts_valid, slots_clean, last_forces_from_table, slots_valid, verlet_ok,
      verlet_tracks_positions, chain_painted;
  long long substep_seq, carry_from;
  int *gathered, *gathered_next;
  long nbsteps;
  double Mdx, Mhy;
  double Mgx, t;   // a vibrating handle's side wall and clock (lbmdem_set_vibration): with nbsteps, where its schedule stands
  long probe_seen, probe_issued;   // the probe recorder's counts (ProbeState): the ring's write and drop counters follow from them
  long tracer_advances, tracer_hook;   // the tracers' counts (TracerState): the advances behind a failed launch did nothing
  int scalar_cur;                      // the passive scalar's ping-pong index and counts (ScalarState): likewise its steps
  long scalar_steps, scalar_hook;
  long mean_samples, mean_hook;        // the time averages' counts (MeanState): the samples behind a failed launch added nothing
};

// Time-averaged flow statistics (lbmdem_mean_*, lbm_mean.hip). Nothing is allocated or launched while no window is open; `every`
// is 0 then, which is all lbmdem_forces_fluid looks at.
struct MeanState {
  bool on = false;
  int mask = 0, every = 0;    // LBMDEM_MEAN_* of the window; every >= 1: the k-th fluid step since the window opened is sampled when k % every == 0
  int nsel = 0;               // planes of doubles the mask selects
  unsigned* cnt = nullptr;    // device [2][lx][sy]: n_fluid, n_grain
  double* S = nullptr;        // device [nsel][lx][sy]: the selected planes in table order
  long samples = 0, hook = 0; // samples in the window; fluid steps the hook has counted (lbmdem_mean_reset keeps it modulo `every`)
  double* out = nullptr;      // [out_cap] scratch of lbmdem_mean_fields and lbmdem_mean_profile
  long out_cap = 0;
  // one shot: the window came out of a checkpoint (lbmdem_checkpoint_load) and nothing has been run on it since.
  // lbmdem_run_scene goes on with such a window instead of opening a new one when it is the window it would open.
  bool resumed = false;
};
// planes of doubles per bit of a window's mask, in table order (Sux Suy | Sxx Sxy Syy | Srho Srho2 | Sdiss Sgdot | Sgux Sguy)
constexpr int MEAN_BIT_PLANES[5] = {2, 3, 2, 2, 2};
static inline int mean_planes_of(int mask) {
  int c = 0;
  for (int b = 0; b < 5; ++b) c += ((mask >> b) & 1) ? MEAN_BIT_PLANES[b] : 0;
  return c;
}

// The passive scalar (lbmdem_scalar_*, lbm_scalar.hip). Nothing is allocated or launched while `on` is false.
struct ScalarState {
  bool on = false;
  bool automatic = false;     // every fluid step steps the field once (lbmdem_forces_fluid, behind the tracer advance)
  double tau = 0., omega = 0.;   // omega = 1. / tau, formed once on the host
  double* g[2] = {nullptr, nullptr};   // device [5][lx][sy] each: the populations, ping-pong; g[cur] is the present state
  int cur = 0;
  unsigned char* was = nullptr;   // device [lx][sy]: the nodes that were fluid when the field was last stepped or set
  double* conc = nullptr;     // device [lx][ly]: the concentration plane of the download, the torch view and the file
  double* part = nullptr;     // [part_cap] scratch of lbmdem_scalar_sums: per (row, block of 64 y) [lx][nb][5], then the rows [lx][5]
  long part_cap = 0;
  double* sums = nullptr;     // [5]
  long steps = 0, hook = 0;   // steps made since lbmdem_scalar_set; those of them the fluid steps made
};

// Fluid tracers (lbmdem_tracer_*, lbm_tracers.hip). Nothing is allocated or launched while n == 0.
// positions (2 doubles) and the sample's scratch (3 doubles) of a set stay under 1 GiB together
constexpr long TRACER_MAX = ((long)1 << 30) / (long)(5 * sizeof(double));
struct TracerState {
  long n = 0;
  bool automatic = false;     // every fluid step advances the set once (lbmdem_forces_fluid, behind the probe sample)
  double* xy = nullptr;       // device [n][2]: px, py in node coordinates, updated in place
  double* uvo = nullptr;      // device [uvo_cap] scratch of lbmdem_tracer_sample and lbmdem_write_tracers: [n][3] U, V, owner
  long uvo_cap = 0;
  long advances = 0, hook = 0;   // advances made since lbmdem_tracer_set; those of them the fluid steps made
};

// The probe recorder (lbmdem_probe_*, lbm_probe.hip). Off unless lbmdem_probe_enable has set it up.
struct ProbeState {
  bool on = false;
  int every = 1, capacity = 0, pressure_row = -1, npoints = 0;
  long rec = 0;               // doubles per record
  long off[6] = {0, -1, -1, -1, -1, -1};   // where each field starts in a record (lbmdem_probe_layout)
  double* ring = nullptr;     // device [capacity][rec]
  long long* ctr = nullptr;   // device {written, dropped} x 2 (k_probe_sample)
  int* points = nullptr;      // device [npoints][2]
  long seen = 0;              // fluid steps since lbmdem_probe_enable (every k-th is sampled)
  long issued = 0;            // samples launched since the ring was last emptied: min(issued, capacity) are in it, the rest were dropped
};

// Frames, tables and checkpoints written in the background (lbmdem_set_async_output, lbmdem_set_async_dem,
// lbmdem_set_async_checkpoint; lbmdem_output.hip). A job is snapshotted on the handle's stream into its slot's device staging
// (k_vtk_frame: the image the files hold; k_dem_frame: the table's rows; k_ckpt_frame: the sections of the file), copied to the
// slot's pinned buffer on the copy stream behind an event, and written by the writer thread once the copy's event has completed.
// A slot is free again when its files are closed: staging and pinned buffer are never overwritten while anything reads them.
// Nothing of this exists while the three features are off.
// The header of a checkpoint's extension (lbmdem_set_checkpoint_contents; the byte layout is in include/lbmdem_hip.h): what the
// host knows of the optional state the file carries. The five sections it announces follow it (CKPT_TABLE, lbmdem_internal.h),
// each absent (length 0) when its bit of `mask` is clear.
struct CkptExtra {
  char magic[8];       // "LBMXTRA1"
  int mask, pad0;      // LBMDEM_CKPT_* of what follows
  long plane;          // sanity: lx * sy of the writer
  long tr_n;           // tracers: TracerState's n, automatic, advances, hook
  int tr_automatic, pad1;
  long tr_advances, tr_hook;
  double sc_tau;       // scalar: ScalarState's tau, automatic, steps, hook (omega is formed from tau again)
  int sc_automatic, pad2;
  long sc_steps, sc_hook;
  int mn_mask, mn_every, mn_nsel, pad3;   // window: MeanState's mask, every, nsel, samples, hook
  long mn_samples, mn_hook;
};
static_assert(sizeof(CkptExtra) == 120, "the extension header has the documented layout");
struct CkptShot {      // the host's side of a checkpoint's header as it stood when the checkpoint was queued. The pair list's
  lbmdem_config cfg;   // length, the carries and the sections' digests come back with the copy (the staging's word area).
  long nbsteps = 0, plane = 0;   // (cfg: incl. the clock and the walls)
  double lid6 = 0;
  int force_mode = 0, diag_always = 0, verlet_ok = 0, vib = 0;
  CkptExtra xtra{};    // mask == 0: the file has no extension
};
struct AsyncSlot {
  void* staging = nullptr;   // device, AsyncLane::bytes
  void* pinned = nullptr;    // host, the same
  hipEvent_t snapped = nullptr, copied = nullptr;
  bool busy = false;         // (under AsyncOut::mu)
  char path[4096];           // the directory; a checkpoint's file name
  // what the job's kind needs besides: the frame's or table's number, the map with the table, the stats.data line as it stood
  // when the event was queued, the checkpoint's header
  int nfile = 0, with_forces = 0;
  double stats22[22];
  // a checkpoint is laid out job by job: optional state can appear or vanish between two queued checkpoints
  CkptShot shot;
  CkptLayout ckpt_layout{};   // where the job's sections lie in staging and pinned buffer
  size_t ckpt_bytes = 0;      // the job's copy: ckpt_layout.total, never more than AsyncLane::bytes
};
// The counters of lbmdem_output_stats / lbmdem_output_stats_dem / lbmdem_output_stats_checkpoint: each kind has its own set,
// reset when its slots change
struct AsyncCounters {
  long queued = 0, written = 0, failed = 0, slot_waits = 0;
  // ms_last: frames -- the caller in lbmdem_output_drain; tables -- the caller waiting for the 22 numbers; checkpoints -- the
  // caller inside lbmdem_checkpoint_save_async behind its slot (header fields, launch, queueing)
  double ms_slot_wait = 0, ms_copy_wait = 0, ms_io = 0, ms_last = 0;
};
enum : int { ASYNC_FRAME = 0, ASYNC_TABLE = 1, ASYNC_CKPT = 2, ASYNC_KINDS = 3 };
static const char* const ASYNC_KIND_NAMES[ASYNC_KINDS] = {"frame", "table", "checkpoint"};
// A kind's slots (0: the kind is off; at most LBMDEM_ASYNC_MAX_FRAMES, _DEM, _CKPT of them), the size of a job's copy, its counters
struct AsyncLane {
  int slots = 0;
  size_t bytes = 0;
  AsyncSlot slot[4];
  AsyncCounters c;
};
static_assert(LBMDEM_ASYNC_MAX_FRAMES <= 4 && LBMDEM_ASYNC_MAX_DEM <= 4 && LBMDEM_ASYNC_MAX_CKPT <= 4, "AsyncLane::slot");
struct AsyncJob { int kind, slot; };
// One per handle while any of the three kinds is on: ONE copy stream, ONE writer thread, ONE queue (strictly first in, first out:
// the lines of stats.data land in call order).
struct AsyncOut {
  int lx = 0, ly = 0, n = 0, device = 0;     // lattice, grains
  // the slots' staging and pinned buffers, dem_scratch, dem_stats_host. Only the thread that calls into the library allocates
  // and frees here (lane_resize, lbmdem_async_release, with the writer idle or joined); the writer thread only reads a slot's
  // pinned buffer and never touches the pool.
  MemPool mem;
  AsyncLane lane[ASYNC_KINDS];
  double* dem_scratch = nullptr;             // device: the addends of the ten sums [10][n], then the 22 numbers (k_dem_stats)
  double* dem_stats_host = nullptr;          // pinned [22]
  hipStream_t copy_stream = nullptr;
  std::thread writer;
  std::mutex mu;
  std::condition_variable cv_job, cv_free;   // writer: a job or quit; callers: a slot freed / a job finished
  std::deque<AsyncJob> jobs;                 // in the order they were queued
  bool quit = false;
  int pending = 0;                           // queued and not yet on disk
  // the first failure of the writer since the last one was reported (the writer never touches the callers' error text)
  int err_code = 0;
  int err_kind = ASYNC_FRAME;                // ... was a frame's, a table's, a checkpoint's
  char err_msg[4400];
};

// Which map and populations a result of the map-reading analyses (pores to netsolve) describes: those of sub-step `seq`, upload
// `moved` and lattice change `fluid`. set() takes the three from the handle and raises `valid`; current() asks for `valid`,
// seq == substep_seq, moved == grains_moved and fluid == lattice_seq (a rasterisation, a fluid step and lbmdem_upload_f raise the
// last). Both are defined in lbm_stage.h, with the rest of what those analyses share.
struct MapStamp {
  bool valid = false;
  long long seq = -1, moved = -1, fluid = -1;
  void set(const lbmdem_handle* h);
  bool current(const lbmdem_handle* h) const;
};

struct lbmdem_handle {
  lbmdem_config cfg;
  LatticeView L;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // every device and pinned block of the handle, the members of V, dd, ct, dx, chain and probe included: lbmdem_destroy frees
  // them in one go; what goes earlier (the probe recorder's buffers) is released by name
  MemPool mem;
  // lattice
  real* f[2] = {nullptr, nullptr};
  int fcur = 0;
  int* obst[2] = {nullptr, nullptr};
  int ocur = 0;           // map the current f was produced with ("old" for the next collide_stream)
  bool obst_pending = false;  // obst[1 - ocur] holds a newer map not yet consumed by collide_stream
  // obst[1 - ocur] -- the map the fused kernel has finished with, the next rasterisation's canvas -- is reset to "no
  // grains" in slices by the DEM sub-step launches (single domain) or all at once by the launch that unpacks the
  // neighbours' messages (C transport): local rows [0, obst_reset_rows) are done; obst_construction does the rest
  int obst_reset_rows = 0;
  // the map updated in place (k_obst_update, lbm_obst.hip): per map buffer the centres its discs were painted at, in two
  // slots (the update reads one and writes the other: partners look at each other's old centres meanwhile)
  ObstSnap snap[2][2] = {};
  int snap_cur[2] = {0, 0};
  bool snap_ok[2] = {false, false};   // snap[b][snap_cur[b]] describes what obst[b] holds
  bool obst_update = true;            // lbmdem_set_obst_update: maps are updated in place where a picture to start from exists
  long obst_updates = 0, obst_repaints = 0;   // lbmdem_obst_stats
  int list_generation = 0;            // rebuilds so far
  volatile int* moved_host = nullptr; // pinned: the generation of the list in which k_obst_update found a grain too far from where the list found it
  int* moved_dev = nullptr;
  // where the two maps of a fluid step differ (ObstChange, lbmdem_internal.h): chg[b] belongs to obst[b] as the NEW map.
  // chg_state[b]: 0 = says nothing, 1 = all clear and nobody has painted obst[b] since, 2 = written by the rasterisation
  // that painted obst[b] in place (k_dem_chain's tail) against the picture in obst[1 - b]
  unsigned* chg[2] = {nullptr, nullptr};
  int chg_state[2] = {0, 0};
  int chg_words = 0, chg_windows = 0, chg_ww = 0, chg_off = 0;
  bool chg_on = true;                 // lbmdem_set_change_mask
  int chg_verify = 0;                 // ... 2: every use is checked against the two maps first (tests)
  long chg_used = 0;                  // fused launches that read one map where the bits allowed it
  int* chg_bad = nullptr;             // device counters of the verification: [0] clear bits over rows that differ, [1] populations
                                      // that come out differently with and without the bits
  real* chg_fcheck = nullptr;         // (mode 2) a second output lattice
  // collide_stream in two parts (lbmdem_collide_stream_part): after EDGES the interior rows of f[fcur] are
  // still missing; the operands of the launch are kept for INTERIOR
  bool cs_interior_pending = false;
  bool cs_prepared = false;   // lbmdem_collide_stream_prepare has run for the coming EDGES part
  const real* cs_fin = nullptr;
  const int *cs_ob_old = nullptr, *cs_ob_new = nullptr;
  int cs_lo_end = 0, cs_hi_begin = 0;  // interior = local rows [cs_lo_end, cs_hi_begin)
  ForceSlots cs_slots{};
  // grains
  int n = 0;
  real* gbuf = nullptr;  // one allocation, carved below
  Kin kin[2];
  int kcur = 0;
  real *r = nullptr, *m = nullptr, *It = nullptr, *rLB = nullptr;
  real *xc = nullptr, *yc = nullptr, *r2 = nullptr, *rbl0 = nullptr;
  real* pk = nullptr;   // [n][8] packed fluid-side grain records
  real* gp = nullptr;   // [n] grain pressure g.p of the last DEM sub-step (main.c:187,776)
  real* diag = nullptr; // [8][n] reals s f1 f2 ifm M11 M12 M21 M22, then [2][n] ints z zz
  bool diag_always = false;
  DiagExtra dx{};          // buffers of the order-dependent diagnostics fr, ice, slip, rw (allocated on first use)
  bool dx_ready = false;
  CarryTrack ct{};            // "previous contact" carries: records left by every ordinary sub-step (single-domain handles)
  long long substep_seq = 0;  // sequence number of the next sub-step (the records' stamps)
  long long carry_from = 0;   // ct.carry is as of the sub-step before this one; only younger records override it
  bool diag_valid = false; // the last sub-step produced diagnostics
  // The contact network export (lbm_contacts.hip). contacts_valid: the last sub-step was a table sub-step and nothing has touched
  // the state it started from (kin[1 - kcur]), its pair list or its wall flags since; contacts_film / contacts_P: the law and the
  // parameters that sub-step was launched with (the walls and the clock may have moved on since). cx: staging, allocated by the
  // first export, grown with the record count, freed with the handle.
  bool contacts_valid = false;
  int contacts_film = 0;
  DemParams contacts_P{};
  // walls_moved: raised whenever Mgx, Mdx, Mby or Mhy takes another value OUTSIDE a sub-step (lbmdem_move_walls,
  // lbmdem_verlet_rebuild, a recovery that puts them back: note_walls below). What was made for the walls as they were is stale
  // then, although no grain has moved: contacts_walls is the count the last table sub-step found (the export and the clusters ask
  // for contacts_walls == walls_moved: walls() no longer describes the walls of their records otherwise), vo.walls the Voronoi
  // compute's. Wall motion inside a run comes with sub-steps, which substep_seq counts.
  long long walls_moved = 0;
  long long contacts_walls = -1;
  bool contacts_output = false;   // lbmdem_set_contacts_output: lbmdem_run_scene writes the contact files at every DEM event
  struct ContactStage {
    int nwg = 0;                          // workgroups of the two kernels (0: nothing allocated yet)
    long long *counts = nullptr, *offsets = nullptr;   // [2 nwg + 1] records per workgroup, pairs then walls; their exclusive scan
    unsigned long long* census = nullptr; // [6]
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
    lbmdem_contact* rec = nullptr;        // [rec_cap]
    long rec_cap = 0;
  } cx;
  // The cluster analysis of the contact net (lbm_clusters.hip). cl: scratch and results, allocated by the first
  // lbmdem_cluster_compute, grown with the record count, freed with the handle. The results describe the table sub-step whose
  // sequence number is `seq`: the readers ask for contacts_valid and seq == substep_seq. clusters_*: lbmdem_set_clusters_output.
  bool clusters_output = false;
  double clusters_fmin = 0.;
  int clusters_relative = 0, clusters_zmin = 0;
  struct ClusterStage {
    bool valid = false;
    long long seq = -1;
    int* ints = nullptr;                  // the per-grain and per-root planes, the scan's flags and positions (null: nothing allocated yet)
    unsigned long long* words = nullptr;  // [5][n] per root: selected pair records, the box's four keys
    unsigned long long* census = nullptr; // [10], then the words of the loops: changed, error
    double* thr = nullptr;                // [1]
    double* partial = nullptr;            // [partial_cap] the block partials of S, then (as long long) the blocks' counts
    long partial_cap = 0;
    unsigned char* sel = nullptr;         // [sel_cap] a record is selected
    long sel_cap = 0;
    lbmdem_cluster* table = nullptr;      // [n / 2 + 1]
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
    long nclusters = 0, npairs = 0, nrec = 0;   // of the last compute
    int rounds_cc = 0, rounds_core = 0;         // rounds the two loops took in the last compute
  } cl;
  // The packing structure beyond contacts (lbm_structure.hip): neighbour shells, g(r), bond order. st: scratch and results,
  // allocated by the first lbmdem_structure_compute, grown with the entries, freed with the handle. The results describe the
  // centres as of sub-step `seq` and upload `moved`: the readers ask for seq == substep_seq and moved == grains_moved (every
  // sub-step raises the one, lbmdem_upload_kinematics the other; a checkpoint load makes a new handle). structure_*:
  // lbmdem_set_structure_output.
  long long grains_moved = 0;
  bool structure_output = false;
  double structure_rcut = 0., structure_shell = 0.;
  int structure_nbins = 0;
  struct StructureStage {
    bool valid = false, listed = false;   // a compute has been made; it made the list, bonds and the four sums too
    long long seq = -1, moved = -1;
    unsigned long long* words = nullptr;  // [ST_WORDS] bounds' keys and the census (null: nothing allocated yet)
    void* grid = nullptr;                 // the cell grid's origin, sides and counts, made on the device
    unsigned* keys = nullptr;             // [2][n] a grain's cell, unsorted and sorted
    int* idx = nullptr;                   // [2][n] the grains, by index and by cell
    double* sorted = nullptr;             // [3][n] x, y, r by cell
    int* ints = nullptr;                  // nb [n + 1], bonds [n], offsets [n + 1]
    double* sums = nullptr;               // [4][n] c6, s6, c2, s2
    double* e2 = nullptr;                 // [4097]
    unsigned long long* hist = nullptr;   // [4096]
    int* nbr = nullptr;                   // [nbr_cap] twice the entries: as emitted, then ascending
    long nbr_cap = 0;
    char* tmp = nullptr;                  // hipcub's scratch, sorts and scan
    long tmp_bytes = 0;
    long entries = 0;                     // of the last compute
    int nbins = 0;
  } st;
  // Voronoi cells (lbm_voronoi.hip): the radical tessellation on top of st's neighbour list. vo: scratch and results, allocated by
  // the first lbmdem_voronoi_compute, the face arrays grown with the faces, freed with the handle. The kernels read st and the
  // kinematics and write here only. seq, moved: as st's, and the readers ask the same of them; walls: the handle's walls_moved at the
  // compute, which clipped every cell with the four walls (the readers ask for walls == walls_moved). voronoi_*:
  // lbmdem_set_voronoi_output.
  bool voronoi_output = false;
  double voronoi_rcut = 0.;
  struct VoronoiStage {
    bool valid = false;
    long long seq = -1, moved = -1, walls = -1;
    unsigned long long* words = nullptr;  // [VO_WORDS] the census (null: nothing allocated yet)
    double* dbl = nullptr;                // [4][n] area, perimeter, phi, R2
    int* ints = nullptr;                  // [4][n] faces, walls, nverts, flags; then nf [n + 1] and foff [n + 1]
    int* rsrc = nullptr;                  // [VOR_MAXV][n] a grain's faces as the cell pass leaves them, face k of grain i at k*n + i
    double* rlen = nullptr;               // [VOR_MAXV][n]
    int* fsrc = nullptr;                  // [fsrc_cap] the faces as CSR
    double* flen = nullptr;               // [flen_cap]
    long fsrc_cap = 0, flen_cap = 0;
    char* tmp = nullptr;                  // hipcub's scratch, the scan
    long tmp_bytes = 0;
    long nfaces = 0;                      // of the last compute
    double rcut = 0.;                     // the structure compute's, as the last compute recovered it
  } vo;
  // Strain fields (lbm_strain.hip): the grains where they are now against a marked reference state. sn: the mark -- a copy of the
  // centres, the angles and st's list, which nothing st or vo do later changes -- and the compute's scratch and results, allocated
  // by the first lbmdem_strain_mark, the list grown with the entries, freed with the handle. The kernels read the mark and the
  // kinematics and write here only. marked: from a successful mark to the next one, lbmdem_strain_clear or the handle's end (steps,
  // uploads and wall moves do not end it; a checkpoint does not carry it); mark_gen counts the marks. The result describes mark
  // `of_mark` and the centres as of sub-step `seq` and upload `moved`: the readers ask for of_mark == mark_gen, seq == substep_seq
  // and moved == grains_moved (walls do not enter). strain_*: lbmdem_set_strain_output.
  bool strain_output = false, strain_incremental = false;
  double strain_rcut = 0.;
  struct StrainStage {
    bool marked = false, valid = false;
    long long mark_gen = 0, of_mark = -1, seq = -1, moved = -1;
    unsigned long long* words = nullptr;  // [SN_WORDS] the census and the argmax (null: nothing allocated yet)
    double* ref = nullptr;                // [3][n] the mark: x1, x2, x3
    int* off = nullptr;                   // [n + 1] the mark: st's offsets
    int* nbr = nullptr;                   // [nbr_cap] the mark: st's list, ascending
    double* rec = nullptr;                // [n][4] the compute's packed records {X0, Y0, x, y}
    double* dbl = nullptr;                // [8][n] ux, uy, drot, Fxx, Fxy, Fyx, Fyy, d2min
    int* ints = nullptr;                  // [3][n] used, lost, flags
    long ref_cap = 0, off_cap = 0, nbr_cap = 0, rec_cap = 0, dbl_cap = 0, ints_cap = 0;
    long entries = 0;                     // of the mark
    double rc2 = 0.;                      // the marked structure compute's rcut*rcut
    long nbsteps = 0;                     // the handle's at the mark
  } sn;
  // The pore space (lbm_pores.hip): the fluid phase labelled into connected components. po: scratch and results, allocated by the
  // first lbmdem_pore_compute, the table grown with the components, freed with the handle. The kernels read the map and f and
  // write here only. The results describe the map and f of po.at (MapStamp), and the readers ask for po.at.current(): lattice_seq
  // is raised by a rasterisation, a fluid step and lbmdem_upload_f. pores_*: lbmdem_set_pores_output.
  long long lattice_seq = 0;
  bool pores_output = false;
  int pores_conn = 8, pores_plane = 0;
  struct PoreStage {
    MapStamp at;                          // the map and populations the last compute was made for
    unsigned long long* words = nullptr;  // [PO_WORDS] the census (null: nothing allocated yet)
    int* parent = nullptr;                // [lx][sy] the union-find: a fluid node's parent, a device node no larger than itself; else -1
    int* label = nullptr;                 // [lx][sy] the result: the smallest host index of the node's component, else -1
    int* rank = nullptr;                  // [lx][sy] at a root: its place in the table (written and read at roots only)
    int* map = nullptr;                   // [lx][sy] a caller's map in device layout (allocated by the first compute that brings one)
    int* cnt = nullptr;                   // [2][nblocks + 1] roots per block of the flatten pass, and their scan
    int* grains = nullptr;                // [3][n] wet, pore_min, pore_max
    lbmdem_pore* table = nullptr;         // [table_cap]
    long table_cap = 0;
    char* tmp = nullptr;                  // hipcub's scratch, the scan
    long tmp_bytes = 0;
    long ncomp = 0;                       // of the last compute
  } po;
  // The pore clearance (lbm_clearance.hip): the exact squared distance from every fluid node to the nearest position that is not
  // fluid, that position's owner, the histogram, the owners' table and the throats. clr: scratch and results, allocated by the
  // first lbmdem_clearance_compute, the ridge records and the throat table grown with their counts, freed with the handle. The
  // kernels read the map and write here only. Valid while clr.at (MapStamp) is current. clearance_*: lbmdem_set_clearance_output.
  bool clearance_output = false;
  int clearance_plane = 0;
  struct ClearanceStage {
    MapStamp at;                          // the map and populations the last compute was made for
    unsigned long long* words = nullptr;  // [CE_WORDS] the census (null: nothing allocated yet)
    unsigned long long* key = nullptr;    // [lx][sy] the row pass: (distance along y)^2 << 32 | owner
    int* d2 = nullptr;                    // [lx][sy] the result: the squared distance, 0 off the fluid and in the pad columns
    int* owner = nullptr;                 // [lx][sy] the result: the nearest position's owner, the map off the fluid, -1 in the pad columns
    int* map = nullptr;                   // [lx][sy] a caller's map in device layout (allocated by the first compute that brings one)
    unsigned long long* hist = nullptr;   // [hbins] fluid nodes per isqrt(d2)
    int hbins = 0;                        // (min(lx, ly) + 1) / 2 + 2: no isqrt(d2) reaches it
    unsigned long long* owned = nullptr;  // [n + 1] fluid nodes per owner
    int* d2max = nullptr;                 // [n + 1] the largest d2 among them, -1 without one
    unsigned long long* cnt = nullptr;    // [2][nblocks + 1] ridge edges per block of the count pass, and their scan
    unsigned long long* rec = nullptr;    // [4][rec_cap] the ridge records: pair keys and values, each with the sort's second buffer
    unsigned long long* uniq = nullptr;   // [rec_cap] the distinct pair keys
    int* runs = nullptr;                  // [2][rec_cap] their run lengths, and the scan of those
    long rec_cap = 0;
    int* nruns = nullptr;                 // [1] the run-length encode's count
    lbmdem_throat* table = nullptr;       // [table_cap]
    long table_cap = 0;
    char* tmp = nullptr;                  // hipcub's scratch: the scans, the sorts, the encode
    long tmp_bytes = 0;
    long nedges = 0, nthroats = 0;        // of the last compute
    int kmax = 0;
    bool own = false;                     // the last compute was of the handle's map, not of a caller's (lbm_network.hip reuses d2 then)
    unsigned long long gen = 0;           // counts the computes: a result made over d2 says which one (lbm_geodesic.hip)
  } clr;
  // The pore network (lbm_network.hip): a watershed of clr.d2 -- per fluid node the body (the local maximum it climbs to) and the
  // group its body merges into, the body and group records and the links of both levels. net: planes and block counts allocated by
  // the first lbmdem_network_compute, the per-body arrays and the tables grown with their counts, freed with the handle; the sort
  // records of a call live in a pool of that call. The kernels read clr.d2 and write here only. Valid under the clearance's guard.
  // network_*: lbmdem_set_network_output.
  bool network_output = false;
  int network_merge = -1, network_plane = 0;
  struct NetworkStage {
    MapStamp at;                          // the map and populations the last compute was made for
    unsigned long long* words = nullptr;  // [NW_WORDS] the census (null: nothing allocated yet)
    int* par = nullptr;                   // [lx][sy] the ascent: a higher node of the same basin, in the end the peak; -1 off the fluid
    int* body = nullptr;                  // [lx][sy] the result: the body's number, -1 off the fluid and in the pad columns
    int* group = nullptr;                 // [lx][sy] the result: the group's root body; before that the peaks' numbers
    unsigned long long* cnt = nullptr;    // [2][nblocks + 1] peaks, then edges, per block of nodes, and their scan
    int* nruns = nullptr;                 // [1] the run-length encode's count
    lbmdem_net_body* bodies = nullptr;    // [body_cap]
    int* barr = nullptr;                  // [5][body_cap + 1] per body: group, degree of either level, root flag and its scan
    unsigned long long* best = nullptr;   // [body_cap] per body the merge candidate, saddle << 32 | ~partner
    long body_cap = 0;
    lbmdem_net_group* groups = nullptr;   // [group_cap]
    long group_cap = 0;
    lbmdem_net_link* links[2] = {nullptr, nullptr};   // [link_cap[level]]
    long link_cap[2] = {0, 0};
    long nbodies = 0, ngroups = 0, nlinks[2] = {0, 0};   // of the last compute
    bool own = false;                     // the last compute was of the handle's map, not of a caller's (lbm_drainage.hip reuses it then)
    unsigned long long gen = 0;           // counts the computes: a result made over the tables says which ones (lbm_drainage.hip)
    int merge = -1;                       // of the last compute (lbm_netflux.hip reuses a result of the same merge)
  } net;
  // Drainage (lbm_drainage.hip): the widest path over clr.d2 from an inlet side -- per fluid node access, per body of the network A,
  // per level-0 link pass, the histogram of isqrt(access). drn: the plane, the histogram and the words allocated by the first
  // lbmdem_drainage_compute, A and pass grown with the network's counts, freed with the handle. The kernels read clr.d2, net.body
  // and net.links[0] and write here only. Valid under the network's guard and while net.gen is the one it was made over.
  // drainage_*: lbmdem_set_drainage_output.
  bool drainage_output = false;
  int drainage_from = 0, drainage_band = 1, drainage_to = 0, drainage_plane = 0;
  struct DrainageStage {
    MapStamp at;                          // the map and populations the last compute was made for
    unsigned long long gen = 0;           // net.gen of the network result underneath
    unsigned long long* words = nullptr;  // [DR_WORDS] the counts and the relaxation's `changed` (null: nothing allocated yet)
    int* access = nullptr;                // [lx][sy] the result: min(d2, A[body]), 0 off the fluid and in the pad columns
    unsigned long long* hist = nullptr;   // [clr.hbins] fluid nodes per isqrt(access)
    int* A = nullptr;                     // [a_cap] per body
    long a_cap = 0;
    int* pass = nullptr;                  // [pass_cap] per level-0 link
    long pass_cap = 0;
    long nbodies = 0, nlinks = 0;         // of the last compute
    int kmax = 0;                         // the clearance's at that compute: the histogram has kmax + 1 bins
    int rounds = 0;                       // launches of the relaxation, the quiet last one included
  } drn;
  // Geodesic (lbm_geodesic.hip): the shortest path through the passable fluid nodes from an inlet region (dist), from an outlet
  // region (back), the corridor between them (detour) and the profile over the depth behind the inlet. geo: the planes, the tile
  // lists and the words allocated by the first lbmdem_geodesic_compute, the profile grown with the depths, freed with the handle.
  // The kernels read the map, or clr.d2 when min_d2 > 1, and write here only. Valid under the pores' guard, and with min_d2 > 1
  // over the handle's map while clr.gen is the one it was made over. geodesic_*: lbmdem_set_geodesic_output.
  bool geodesic_output = false;
  int geodesic_from = 0, geodesic_band = 1, geodesic_to = 0, geodesic_conn = 8, geodesic_min_d2 = 0, geodesic_plane = 0;
  struct GeodesicStage {
    MapStamp at;                          // the map and populations the last compute was made for
    bool over_clearance = false;          // made over clr.d2 of the handle's map
    unsigned long long gen = 0;           // ... clr.gen of that result
    unsigned long long* words = nullptr;  // [GEO_WORDS] the counts (null: nothing allocated yet)
    int* dist = nullptr;                  // [lx][sy] the result: the distance from the inlet, -1 where not passable or not reached and in the pad columns
    int* back = nullptr;                  // [lx][sy] the same from the outlet
    int* detour = nullptr;                // [lx][sy] dist + back - shortest
    int* map = nullptr;                   // [lx][sy] a caller's map in device layout (allocated by the first compute that brings one)
    int* stamp = nullptr;                 // [tiles] the round a tile of the relaxation was last listed for
    int* list = nullptr;                  // [2][tiles] the active tiles of this round and of the next
    unsigned* cnt = nullptr;              // [2] their lengths
    unsigned long long* lev = nullptr;    // [3][depths] per depth: passable nodes, reached ones, the sum of dist
    long lev_cap = 0;
    int* lmm = nullptr;                   // [2][depths] per depth: the least and the largest dist
    long lmm_cap = 0;
    std::vector<lbmdem_geo_level> levels; // the profile of the last compute, on the host
    int rounds[2] = {0, 0};               // launches of the forward and the backward relaxation, the quiet last ones included
  } geo;
  // Pore fluxes (lbm_netflux.hip): the mass that crossed every edge of adjacent fluid nodes in the last streaming step, in fixed
  // point, per link and region of the network's `level` and per section of the lattice. nfx: the profiles and the words allocated
  // by the first lbmdem_netflux_compute, the tables grown with the network's counts, freed with the handle. The kernels read f,
  // net.body or net.group and net.links[level] and write here only. Valid under the pores' guard (lattice_seq covers f) and while
  // net.gen is the one it was made over. netflux_*: lbmdem_set_netflux_output.
  bool netflux_output = false;
  int netflux_merge = -1, netflux_level = 0;
  struct NetfluxStage {
    MapStamp at;                          // the map and populations the last compute was made for
    unsigned long long gen = 0;           // net.gen of the network result underneath
    unsigned long long* words = nullptr;  // [NF_WORDS] the counts (null: nothing allocated yet)
    long* col = nullptr;                  // [lx] the sections towards +x: lx - 1 of them
    long* row = nullptr;                  // [ly] the sections towards +y: ly - 1 of them
    int* first = nullptr;                 // [first_cap] per body number the first link with lo >= it
    long first_cap = 0;
    unsigned long long* sums = nullptr;   // [3][bodies] mass, net and through by body number
    long sums_cap = 0;
    lbmdem_netflux_link* links = nullptr; // [link_cap] aligned with net.links[level]
    long link_cap = 0;
    lbmdem_netflux_region* regions = nullptr;   // [region_cap] aligned with net.bodies or net.groups
    long region_cap = 0;
    long nlinks = 0, nregions = 0;        // of the last compute
    int merge = -1, level = 0;
  } nfx;
  // Network pressures (lbm_netsolve.hip): the pore network of `level` as a resistor network between the regions on an inlet side
  // (p = 1) and those on an outlet side (p = 0), solved by a Jacobi-preconditioned conjugate gradient whose every operation the
  // header spells out. nsv: the words allocated by the first lbmdem_netsolve_compute, everything else grown with the network's
  // counts, freed with the handle. The kernels read net.body or net.group, the tables of the level and write here only. Valid
  // under the network's guard and while net.gen is the one it was made over. netsolve_*: lbmdem_set_netsolve_output.
  bool netsolve_output = false;
  int netsolve_merge = -1, netsolve_level = 0, netsolve_from = 0, netsolve_band = 1, netsolve_to = 0, netsolve_max_iter = 0;
  double netsolve_rtol = 1e-8;
  struct NetsolveStage {
    MapStamp at;                          // the map and populations the last compute was made for
    unsigned long long gen = 0;           // net.gen of the network result underneath
    unsigned long long* words = nullptr;  // [NS_WORDS] status, iterations and the counts (null: nothing allocated yet)
    double* scal = nullptr;               // [NS_SCAL] rz0, the last rz, rz of the iteration (two), Q_in, Q_out
    int* lints = nullptr;                 // [7][L'] per link: the two regions, the sort's three arrays; the rows' partners (2 L')
    long lint_cap = 0;
    double* ldbl = nullptr;               // [4][L'] per link: g; the rows' g (2 L'); the caller's g
    long ldbl_cap = 0;
    int* rints = nullptr;                 // [3][R'] per region: the two firsts of its row, its flags
    long rint_cap = 0;
    double* rdbl = nullptr;               // [8][R'] per region: diag, b, x, r, z, q and d twice
    long rdbl_cap = 0;
    unsigned* bits = nullptr;             // [bits_cap] by body number: an inlet node 1, an outlet node 2
    long bits_cap = 0;
    double* parts = nullptr;              // [4][P'] per block of 256 regions: its part of dq, of dot(r, z), of Q_in, of Q_out
    long part_cap = 0;
    lbmdem_netsolve_link* links = nullptr;      // [link_cap] aligned with net.links[level]
    long link_cap = 0;
    lbmdem_netsolve_region* regions = nullptr;  // [region_cap] aligned with net.bodies or net.groups
    long region_cap = 0;
    char* tmp = nullptr;                  // hipcub's scratch: the sort
    long tmp_bytes = 0;
    long nlinks = 0, nregions = 0;        // of the last compute
    int rounds = 0;                       // launches of the iteration in the last compute
  } nsv;
  // Coarse-grained fields (lbm_coarse.hip). coarse_cw, coarse_ch: lbmdem_set_coarse_output's cell size, 0 x 0 is off. cg: scratch,
  // allocated by the first export, grown when a finer grid needs more, freed with the handle.
  int coarse_cw = 0, coarse_ch = 0;
  struct CoarseStage {
    double *cells = nullptr, *col = nullptr;   // [cell_cap] the records, 25 doubles per cell; [col_cap] column sums, [lx][7][ncy]
    long cell_cap = 0, col_cap = 0;
    unsigned* keys[2] = {nullptr, nullptr};    // [n] the grains' cells, unsorted and sorted (null: nothing allocated yet)
    int* idx[2] = {nullptr, nullptr};          // [n] ... and their indices
    long long* outside = nullptr;              // [1]
    void* sort_tmp = nullptr;
    long sort_bytes = 0;
  } cg;
  // Flow fields (lbm_flow.hip). flow_output: lbmdem_set_flow_output. fl: scratch, allocated by the first call that needs it, grown
  // when a call asks for more, freed with the handle.
  bool flow_output = false;
  struct FlowStage {
    double* planes = nullptr;   // [planes_cap] the selected planes of a host export, [lx][ly] each
    long planes_cap = 0;
    double* part = nullptr;     // [part_cap] per (row, block of 64 y) partial sums, [lx][nb][8]; then the row sums [lx][8]
    long part_cap = 0;
    double* sums = nullptr;     // [8]
    unsigned* image = nullptr;  // [image_cap] the payloads of flow%.6i.vtk in file byte order, 6 words per node
    long image_cap = 0;
  } fl;
  real* fhf = nullptr;  // [3][n]
  unsigned char* owner = nullptr;
  unsigned* mincov = nullptr;   // GrainFluidView::mincov
  unsigned paint_epoch = 0;
  // the map buffer that xc, yc, r2, rbl0 and the mincov record describe: the one the most recent rasterisation painted (what
  // the boundary-link export shows, lbm_links.hip). -1: none -- the picture those centres belong to has been given up
  // (drop_chain_paint, a launch of k_dem_chain undone) or replaced (a loaded checkpoint's map)
  int geo_buf = -1;
  // link sums handed from the fused kernel to the force kernel (ForceSlots, lbmdem_internal.h)
  ForceSlots fs{};
  int* gathered2 = nullptr;   // both counters (fs.gathered / fs.gathered_next alternate between them)
  bool slots_clean = false;  // every slot is empty
  bool last_forces_from_table = false;
  bool slots_valid = false;  // the table was filled by the collide_stream that produced f[fcur] with the current map
  double rmax = 0.0, rmin = 0.0;
  // strip decomposition with distributed grains (lbmdem_dist_*)
  bool dist = false, dist_poison = false;
  bool dist_period_open = false;   // lbmdem_dist_begin_period has classified the grains for the coming fluid step
  int dist_margin = 0;
  DistDevice dd{};
  VerletDevice V{};
  bool verlet_ok = false;
  bool verlet_tracks_positions = false;  // the positions have only moved by DEM sub-steps since the list was built (no upload)
  volatile int* ovf_host = nullptr;  // pinned mirror of V.overflow, refreshed (asynchronously) after every rebuild
  volatile int* ferr_host = nullptr; // pinned mirror of fs.error (strip decomposition), refreshed by every period's classification launch
  int* ferr_mirror = nullptr;        // ... its device address
  // runs of ordinary sub-steps in one launch (k_dem_chain, dem_kernels.hip)
  DemChain chain{};
  int chain_max = 128;         // longest run handed to one launch; < 2: one launch per sub-step (lbmdem_set_dem_chain)
  bool chain_checked = false;  // the residency census has run (chain.capacity says what it found)
  long chain_launches = 0, chain_substeps = 0;   // lbmdem_dem_chain_stats
  // the run of sub-steps that ended at a fluid step has rasterised the discs into obst[1 - ocur] itself (ChainPaint): the
  // next obst_construction has nothing to launch. Dropped (and the canvas marked dirty) by whatever moves a grain first.
  bool chain_painted = false;
  bool chain_paint = true;     // (lbmdem_set_dem_chain: max_substeps < 0 switches only this off, for A/B)
  real chain_paint_Mgx = 0.;   // the side wall the discs were painted against (vibrating walls move it)
  long chain_paints = 0;
  int dem_tiles_mode = 0;      // how the tiles of k_dem_chain are composed (lbmdem_set_dem_tiles)
  // launches of k_dem_chain that have not been seen to finish, the calls they belong to, and how often one had to be undone
  std::vector<ChainSnap> chain_pending;
  std::vector<RunLogEntry> runlog;
  int in_run = 0;              // inside lbmdem_run / lbmdem_run_dem (their pieces do not settle on their own)
  bool run_logged = false;     // ... of a call that is in the log (a replay is not)
  long chain_recoveries = 0;
  int chain_giveup_at = -1;    // (experiment build: the launch, counted from 0, that is made to give up; lbmdem_debug_chain_giveup)
  long nbsteps = 0;
  ProbeState probe;
  TracerState tracers;
  bool tracer_output = false;   // lbmdem_set_tracer_output: lbmdem_run_scene writes tracers%.6i.vtk at every VTK event
  ScalarState scalar;
  bool scalar_output = false;   // lbmdem_set_scalar_output: lbmdem_run_scene writes scalar%.6i.vtk at every VTK event, a line of scalar.data at every DEM event
  // write_densities (lbm_densities.hip): the staging budget in bytes (0: the default) and, of the last call, the bytes of the
  // two sections, the bands, the nodes the device refused to format (lbmdem_densities_stats)
  size_t dens_budget = 0;
  long dens_stats[4] = {0, 0, 0, 0};
  MeanState mean;
  int mean_output_mask = 0, mean_output_every = 0;   // lbmdem_set_mean_output: lbmdem_run_scene opens a window and writes mean%.6i.vtk, mean_profile%.6i.dat at every VTK event
  AsyncOut* aout = nullptr;   // null: frames, tables and checkpoints are written synchronously (the default)
  // lbmdem_set_checkpoint_every: lbmdem_run_scene saves to ckpt_path whenever the step counter reaches a multiple (0: never)
  long ckpt_every = 0;
  char ckpt_path[4096] = "";
  int ckpt_contents = 0;   // lbmdem_set_checkpoint_contents: the LBMDEM_CKPT_* every save adds where the handle has them (0: none)
  // KE, PE, SE, IFR, WF, INCE, TSLIP, TRW of the last write_DEM of lbmdem_run_scene: its "steps" line prints them (main.c:1885-1889)
  double scene_energies[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int force_mode = 0;
  // vibrating side walls (lbmdem_set_vibration, main.c:1700-1705): cfg.phys.t, cfg.Mgx and cfg.Mdx advance on the host as
  // sub-steps are issued (vib_advance; with nbsteps they say where the schedule stands); a launch of k_dem_chain reads its sub-steps' walls from a table (DemParams::vib)
  // copied from a pinned ring on the handle's stream. The ring has two halves; a half is written again only after the event
  // recorded behind the last launch that read it has completed.
  bool vib = false;
  VibWall* vib_host = nullptr;  // pinned [2][VIB_HALF]
  VibWall* vib_dev = nullptr;   // device [2][VIB_HALF]
  int vib_half = 0, vib_off = 0;
  hipEvent_t vib_ev[2] = {nullptr, nullptr};
  bool vib_ev_set[2] = {false, false};
  // derived scalars
  double fscale12 = 0, fscale3 = 0;
  double* dpartial = nullptr;
  // profiling of the dominant kernel
  bool prof = false;
  int prof_stride = 1;      // every prof_stride-th launch of the fused kernel is timed (two event records cost the step ~10 us)
  long prof_count = 0;
  bool prof_this = false;   // the launch being issued is one of them
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<hipEvent_t> ev2;      // end of the EDGES part of a split launch (it may run on another stream, next to INTERIOR)
  std::vector<char> ev2_set;
  size_t ev_used = 0;
};

// Every entry point starts here. Outside lbmdem_run / lbmdem_run_dem a handle with unconfirmed launches of k_dem_chain is
// settled first: the stream is drained and, if one of them gave up, the state is taken back to that launch and the calls since
// are replayed (so a download, a checkpoint, a file writer, an upload never meet a state that a failed launch left behind).
#define CHECK_H(h) do { if (!(h)) return fail(LBMDEM_EINVAL, "null handle"); HIP_TRY(hipSetDevice((h)->cfg.device)); \
                        if (!(h)->in_run && !(h)->chain_pending.empty()) RC_TRY(lbmdem_chain_settle(h)); } while (0)
#define CHECK_H_RUNNING(h) do { if (!(h)) return fail(LBMDEM_EINVAL, "null handle"); HIP_TRY(hipSetDevice((h)->cfg.device)); } while (0)
#define CHECK_NOT_SPLIT(h) do { if ((h)->cs_interior_pending) return fail(LBMDEM_EINVAL, "lbmdem_collide_stream_part(LBMDEM_CS_INTERIOR) has not been called after LBMDEM_CS_EDGES"); } while (0)

// (distributed handles only: a rank cannot go back on its own -- its neighbours have moved on; single-domain handles recover)
#define CHAIN_FAILED(h) ((h)->chain.err_host && *(h)->chain.err_host)
#define CHAIN_FAIL_MSG "a launch of the multi-sub-step DEM kernel could not finish on this rank (workgroups not co-resident?): every kernel behind it was held back, the rank's state is that of the launch's first sub-step; restart the decomposition from its last checkpoint with lbmdem_set_dem_chain(h, 0)"

// Named ranges for rocprofv3 --marker-trace around the phases of a step (LBMDEM_ROCTX=1; lbmdem_capi.hip)
struct PhaseRange {
  bool on;
  explicit PhaseRange(const char* name);
  ~PhaseRange();
};

// Host buffers at the ABI are double in both builds; the device holds `real`. (Every float is a double: downloads are
// exact; uploads of values that are not floats are rounded to nearest, like an assignment to `real` in the reference.)
static inline hipError_t h2d_real(real* dst, const double* src, size_t n, hipStream_t st) {
#ifdef LBMDEM_SINGLE_PRECISION
  std::vector<real> tmp(n);
  for (size_t k = 0; k < n; ++k) tmp[k] = (real)src[k];
  hipError_t e = hipMemcpyAsync(dst, tmp.data(), sizeof(real) * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // tmp dies here
  return e;
#else
  return hipMemcpyAsync(dst, src, sizeof(real) * n, hipMemcpyHostToDevice, st);
#endif
}
static inline hipError_t d2h_real(double* dst, const real* src, size_t n, hipStream_t st) {
#ifdef LBMDEM_SINGLE_PRECISION
  std::vector<real> tmp(n);
  hipError_t e = hipMemcpyAsync(tmp.data(), src, sizeof(real) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) for (size_t k = 0; k < n; ++k) dst[k] = tmp[k];
  return e;
#else
  hipError_t e = hipMemcpyAsync(dst, src, sizeof(real) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
#endif
}
// The float build covers the step path and the state transfers (what its parity tests and its bench line use); the
// file writers, checkpoints, the strip decomposition and the RCCL transport exist in the double build only.
#ifdef LBMDEM_SINGLE_PRECISION
#define SP_UNAVAILABLE(what) return fail(LBMDEM_EINVAL, what " is not available in the single-precision build of the library")
#else
#define SP_UNAVAILABLE(what) do { } while (0)
#endif
// the whole body of an entry point that takes a handle and exists in the double build only (the float build's stub)
#define SP_REFUSE(h, what) do { if (!(h)) return fail(LBMDEM_EINVAL, "null handle"); SP_UNAVAILABLE(what); } while (0)

static inline GrainFluidView gview(const lbmdem_handle* h) {
  const Kin& K = h->kin[h->kcur];
  return GrainFluidView{K.x1, K.x2, K.v1, K.v2, K.v3, h->xc, h->yc, h->r2, h->rbl0, h->pk, h->mincov, h->paint_epoch};
}
// What an export, a frame or a cadence's setter says to a handle that does not hold everything -- a strip of a decomposition,
// distributed grains -- in the name of the entry point `who`; `instead`: what the owner of such a handle calls in its place.
static inline int whole_handle(const lbmdem_handle* h, const char* who, const char* instead = nullptr) {
  const LatticeView& L = h->L;
  if (L.xo0 == 0 && L.xo1 == L.lx && L.gx0 == 0 && !h->dist) return LBMDEM_OK;
  return fail(LBMDEM_EINVAL, "%s needs the whole lattice and all grains on this handle (not a strip of a decomposition, no "
                             "distributed grains)%s%s", who, instead ? ": " : "", instead ? instead : "");
}
// The obstacle map a reader should see: the one obst_construction has made for the coming fluid step where there is one, else
// the one the last fluid step took (lbmdem_download_obst, the frames, every export of the fluid's fields).
static inline const int* reader_obst(const lbmdem_handle* h) { return h->obst_pending ? h->obst[1 - h->ocur] : h->obst[h->ocur]; }

static inline DemParams dem_params_of(const lbmdem_config& c) {
  const lbmdem_physics& p = c.phys;
  DemParams P;
  P.gate = nullptr;
  P.n = c.nbgrains; P.dt = (real)c.dt; P.dt2 = (real)c.dt2;
  P.kg = (real)p.kg; P.nug = (real)p.nug; P.kt = (real)p.kt; P.mu = (real)p.mu; P.murf = (real)p.murf;
  P.km = (real)p.km; P.num = (real)p.num; P.ktm = (real)p.ktm; P.mumb = (real)p.mumb; P.mum = (real)p.mum; P.nugt = (real)p.nugt;
  P.Mgx = (real)c.Mgx; P.Mdx = (real)c.Mdx; P.Mby = (real)c.Mby; P.Mhy = (real)c.Mhy;
  {
    const real amp = (real)p.amp, freq = (real)p.freq, t = (real)p.t;   // main.c:163-165
    P.wallT_vel = amp * freq * cos((double)(freq * t));                 // main.c:855: cos() is <math.h>'s
  }
  P.xG = (real)c.xG; P.yG = (real)c.yG;
  P.distVerlet = (real)p.distVerlet;
  P.vib = nullptr;
  return P;
}
static inline DemParams dem_params(const lbmdem_handle* h) {
  DemParams P = dem_params_of(h->cfg);
  P.gate = h->chain.gate;
  P.n = h->n;
  return P;
}

// ---- vibrating side walls (main.c:1700-1705); host arithmetic, <math.h>'s sin and cos, no contraction ----
constexpr int VIB_HALF = 1024;   // entries per half of the ring: the longest run of sub-steps a vibrating handle hands to one launch
// renderScene's first block when vib == 1 (main.c:1700-1705): the clock advances by dt, then the left and the right wall
// each move by amp times the sine of freq times the new clock
static inline void vib_step(lbmdem_config& c) {
#pragma clang fp contract(off)
  c.phys.t = c.phys.t + c.dt;
  c.Mgx = c.Mgx + c.phys.amp * sin(c.phys.freq * c.phys.t);
  c.Mdx = c.Mdx + c.phys.amp * sin(c.phys.freq * c.phys.t);
}
// VerletWall's reset of the right and top walls (main.c:1555-1561), at the rebuild of sub-step `nbsteps`
static inline void verlet_wall_reset(lbmdem_config& c, long nbsteps) {
  if (nbsteps * c.dt < c.phys.dtt) {
    c.Mdx = 1.e-3 * c.lx / 10;
    c.Mhy = (1.e-3 * c.ly / 10);
  } else {
    c.Mdx = 1.e-3 * c.lx;
    c.Mhy = 1.e-3 * c.ly;
  }
}
// The four walls, to be compared on the bits, and what every entry point that moves a wall outside a sub-step does afterwards:
// a wall that has taken another value makes stale what was computed with the walls as they were (lbmdem_handle::walls_moved);
// walls that are where they were leave everything readable.
struct WallBits { unsigned long long w[4]; };
static inline WallBits wall_bits(const lbmdem_config& c) {
  const double v[4] = {c.Mgx, c.Mdx, c.Mby, c.Mhy};
  WallBits b;
  memcpy(b.w, v, sizeof v);
  return b;
}
static inline void note_walls(lbmdem_handle* h, const WallBits& before) {
  const WallBits now = wall_bits(h->cfg);
  if (memcmp(now.w, before.w, sizeof now.w) != 0) h->walls_moved++;
}
// the walls a sub-step sees, as dem_params() hands them to the kernels
static inline VibWall vib_wall(const lbmdem_config& c) {
  const DemParams P = dem_params_of(c);
  return VibWall{P.Mgx, P.Mdx, P.wallT_vel};
}

// shared between the translation units
#define LBMDEM_INTERNAL extern "C" __attribute__((visibility("hidden")))
LBMDEM_INTERNAL int lbmdem_write_vtk_file(const char* path, int nx, int ny, const char* name, int dim, const float* data);
LBMDEM_INTERNAL void lbmdem_vtk_put_mesh(FILE* fp, int nx, int ny);   // lbmdem_output.hip: header, mesh, CELL_DATA / POINT_DATA lines
LBMDEM_INTERNAL void lbmdem_ps_head(FILE* fp, int n, const double* x1, const double* x2, const double* r, const double* fm,
                                    size_t stride, int lx, int ly);   // lbm_contacts.hip: header and discs of DEM%06d.ps
// lbm_contacts.hip: count, scan, total and -- when the records fit into `room` -- emit, the records left in h->cx.rec on the device
LBMDEM_INTERNAL int lbmdem_contacts_records(lbmdem_handle* h, const char* who, long room, long* npairs, long* total);
LBMDEM_INTERNAL int lbmdem_verlet_build_lists(lbmdem_handle* h);
LBMDEM_INTERNAL int lbmdem_chain_settle(lbmdem_handle* h);
LBMDEM_INTERNAL int lbmdem_dem_tiles_by_index(lbmdem_handle* h);
// the probe recorder (lbm_probe.hip): one sample behind the force kernels of a fluid step; the device counters of the ring
// set to what probe.issued says (after chain_restore has taken it back)
LBMDEM_INTERNAL int lbmdem_probe_sample(lbmdem_handle* h, const int* obst);
LBMDEM_INTERNAL int lbmdem_probe_sync_counters(lbmdem_handle* h);
// the tracers (lbm_tracers.hip): one advance of the set in the state the stream has reached, `obst` the map to read; `hook`: made
// by a fluid step (lbmdem_forces_fluid, behind the probe sample). Launches on the handle's stream, does not synchronise.
LBMDEM_INTERNAL int lbmdem_tracer_launch(lbmdem_handle* h, const int* obst, bool hook);
// the passive scalar (lbm_scalar.hip): one step of the field in the state the stream has reached, `obst` the map to read; `hook`:
// made by a fluid step (lbmdem_forces_fluid, behind the tracer advance). Launches on the handle's stream, does not synchronise.
// ... and lbmdem_set_scalar_output's line of <dir>/scalar.data (lbmdem_run_scene, at a DEM event)
LBMDEM_INTERNAL int lbmdem_scalar_launch(lbmdem_handle* h, const int* obst, bool hook);
LBMDEM_INTERNAL int lbmdem_scalar_data_line(lbmdem_handle* h, const char* dir);
// the time averages (lbm_mean.hip): the hook of a fluid step (lbmdem_forces_fluid, behind the scalar step; called only while a
// window with every >= 1 is open) counts the step and launches its sample when it is due, `obst` the map to read. Launches on the
// handle's stream, does not synchronise.
LBMDEM_INTERNAL int lbmdem_mean_hook(lbmdem_handle* h, const int* obst);
// background frames and tables (lbmdem_output.hip): every queued job on disk, the writer joined, everything freed (-> off); the
// writer's first unreported failure, if any, as this thread's error (LBMDEM_OK when there is none)
LBMDEM_INTERNAL void lbmdem_async_release(lbmdem_handle* h);
// ... and every queued job on disk, nothing else touched (the writer's failure, if any, stays for lbmdem_async_report)
LBMDEM_INTERNAL void lbmdem_async_wait_idle(lbmdem_handle* h);
static inline bool lane_on(const lbmdem_handle* h, int kind) { return h->aout && h->aout->lane[kind].slots > 0; }
static inline bool async_frames_on(const lbmdem_handle* h) { return lane_on(h, ASYNC_FRAME); }
static inline bool async_dem_on(const lbmdem_handle* h) { return lane_on(h, ASYNC_TABLE); }
static inline bool async_ckpt_on(const lbmdem_handle* h) { return lane_on(h, ASYNC_CKPT); }
// lbmdem_checkpoint.hip, for the background writer (lbmdem_output.hip): what a slot's launch reads, and the file of a slot
// whose copy has arrived -- header, sections, digest trailer to `<path>.tmp`, then renamed onto `<path>`; on failure the text
// goes to `msg`, the .tmp file is removed and `<path>` is not touched
// lbmdem_ckpt_shot: the host's side of the header of the handle as it stands, with the extension header -- what
// lbmdem_set_checkpoint_contents selects and the handle has (C->xtra.mask == 0: none) -- and the layout of that file in a slot
LBMDEM_INTERNAL CkptLayout lbmdem_ckpt_shot(const lbmdem_handle* h, CkptShot* C);
LBMDEM_INTERNAL void lbmdem_ckpt_frame_job(const lbmdem_handle* h, const CkptLayout& Y, unsigned char* staging, CkptFrameJob* J);
LBMDEM_INTERNAL int lbmdem_ckpt_save_replacing(lbmdem_handle* h, const char* path);
LBMDEM_INTERNAL int lbmdem_ckpt_write_slot(const AsyncSlot* S, char* msg, size_t msglen);
LBMDEM_INTERNAL int lbmdem_async_report(lbmdem_handle* h);
// the next obst_construction will update obst[1 - ocur] in place: nobody resets that canvas beforehand
static inline bool obst_update_planned(const lbmdem_handle* h) {
  return h->obst_update && !h->vib && !h->dist && h->snap_ok[1 - h->ocur] && h->verlet_ok && h->verlet_tracks_positions &&
         !*h->ovf_host && h->obst_reset_rows == 0 && *h->moved_host != h->list_generation;
}
// the coming ordinary sub-steps that nothing separates (fluid step when `fluid`, list rebuild, film law, table sub-step), at
// most `remaining`; 0 when the run is shorter than 2 or the multi-sub-step kernel cannot be used -- and that many sub-steps
LBMDEM_INTERNAL long lbmdem_dem_chain_length(lbmdem_handle* h, long remaining, int fluid);
LBMDEM_INTERNAL int lbmdem_dem_chain(lbmdem_handle* h, long k, int fluid);   // fluid: a fluid step may follow (the run may rasterise for it)
static inline void drop_chain_paint(lbmdem_handle* h) {
  if (h->chain_painted) { h->chain_painted = false; h->obst_reset_rows = 0; h->geo_buf = -1; }   // (the canvas holds a picture nobody will use)
}
// pieces of the fluid step for the C transport (lbmdem_comm.hip), which runs the edge rows on its halo lane's stream:
LBMDEM_INTERNAL int lbmdem_collide_stream_prepare(lbmdem_handle* h);
LBMDEM_INTERNAL int lbmdem_collide_stream_part_on(lbmdem_handle* h, int part, hipStream_t st);   // part on stream `st`
LBMDEM_INTERNAL int lbmdem_dist_begin_period_packed(lbmdem_handle* h, void* kin_lo, void* kin_hi);
LBMDEM_INTERNAL int lbmdem_dist_unpack_tables_kin_fill(lbmdem_handle* h, const void* tab_lo, const void* tab_hi,
                                                       const void* kin_lo, const void* kin_hi);
LBMDEM_INTERNAL int lbmdem_vtk_place_block(float* fields11, int lx, int ly, int x0, int nx, const float* block11);
LBMDEM_INTERNAL int lbmdem_dist_enable_caps(lbmdem_handle* h, int M, long cap_g, long cap_t, long cap_l);
LBMDEM_INTERNAL int lbmdem_comm_rank_world(lbmdem_comm* c, int* rank, int* world);   // for lbmdem_run_scene (lbmdem_scene.hip)
