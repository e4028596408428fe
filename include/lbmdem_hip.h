/*
 * lbmdem_hip.h -- C ABI of the MI355X-native 2D LBM-DEM hot path (liblbmdem_hip.so).
 *
 * Drop-in boundary. The reference (cb-geo/2d-lbm-dem, src/main.c) has no plugin/FFI interface:
 * its seam is the set of `void fn(void)` routines that renderScene() (main.c:1697-1777) calls on
 * file-scope globals. Each entry point below replaces one of those call sites; the reference line
 * it stands in for is cited next to it. INTEGRATION.md shows the edit a maintainer of the reference
 * would make to main.c to call this library instead of its own loops.
 *
 * Conventions: plain C types only; every function returns 0 on success and a negative
 * LBMDEM_E* code on failure (lbmdem_last_error() gives the text); no exceptions cross the ABI;
 * the library owns all device memory, the caller owns every host buffer; one host thread per
 * handle. Host-side lattice data uses the REFERENCE layout f[x][y][q], x slow (main.c:56,1802);
 * the device layout (tiles of 16 consecutive y with the nine directions of a tile contiguous,
 * f[x][y / 16][q][y % 16]) is internal.
 *
 * There is no CPU fallback: every entry point fails with LBMDEM_ENODEVICE when no HIP device
 * is usable.
 */
#ifndef LBMDEM_HIP_H
#define LBMDEM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference fixes its lattice with the object-like MACROS lx, ly and scale (main.c:24-32; its benchmark passes
 * them as -Dlx= -Dly= -Dscale=, benchmark.xml:85) and its run length with the macro duration (main.c:47). They would
 * rewrite the member and parameter names below, so they are parked while this header is read and restored at its end:
 * the header can be included anywhere in the reference's main.c (found by compiling the binding of INTEGRATION.md: oracle/make_integration_check.py). */
#pragma push_macro("lx")
#pragma push_macro("ly")
#pragma push_macro("scale")
#pragma push_macro("duration")
#undef duration
#undef lx
#undef ly
#undef scale

#define LBMDEM_OK 0
#define LBMDEM_EINVAL (-1)    /* bad argument / bad state */
#define LBMDEM_ENODEVICE (-2) /* no usable HIP device */
#define LBMDEM_EHIP (-3)      /* a HIP runtime call failed */
#define LBMDEM_ENOMEM (-4)

typedef struct lbmdem_handle lbmdem_handle;

/* Physics constants: the initialised globals of main.c:74-118,143,163-165. */
typedef struct lbmdem_physics {
  double rho_moy, tau, s2, s3, s5, s7, s8, s9, nu, reductionR; /* main.c:74-94  */
  double G, angleG;                                            /* main.c:97-98  */
  double km, kg, kt, ktm, nug, num, nugt;                      /* main.c:104-109 */
  double mu, mum, mumb, murf;                                  /* main.c:110-113 */
  double distVerlet, dtt, iterDEM;                             /* main.c:115-118 */
  double freq, amp, t;                                         /* main.c:163-165 */
  int updateVerlet;                                            /* main.c:116 */
  int stepFilm;                                                /* main.c:143 */
} lbmdem_physics;

/* Run configuration. The derived block is what main() computes at main.c:1836-1860; fill it with
 * lbmdem_derive() (bit-identical arithmetic) or by hand. */
typedef struct lbmdem_config {
  int lx, ly;         /* global lattice (reference macros lx, ly, main.c:27-32) */
  int x_begin, x_end; /* owned strip [x_begin, x_end) of the global lattice; 0, lx on one GPU */
  int halo;           /* extra rows kept beyond each interior cut (0 on one GPU) */
  int device;         /* HIP device ordinal */
  int nbgrains;
  double scale;       /* reference macro `scale` (main.c:24-26) */
  /* derived (main.c:1836-1860) */
  double dx, dtLB, c, dt, dt2;
  int npDEM;
  double Mgx, Mdx, Mby, Mhy; /* wall positions (main.c:201-204,1836-1839) */
  double xG, yG;             /* gravity components (main.c:1841-1842) */
  lbmdem_physics phys;
} lbmdem_config;

/* defaults = the reference's initialisers */
int lbmdem_physics_defaults(lbmdem_physics* p);

/* Time-step derivation, main.c:1836-1860: dx, dtLB, dtmax, npDEM, c, dt from lx, ly, scale and the
 * smallest radius (r in metres). Also sets walls and gravity. Uses cfg->phys. */
int lbmdem_derive(lbmdem_config* cfg, int lx, int ly, double scale, int nbgrains, const double* r);

/* Sample reader, main.c:609-639 (read_sample): comment line, count, then count x "r x y[;]" in
 * units of 1 mm. Returns metres. Arrays are malloc'ed; release with lbmdem_free_host(). */
int lbmdem_read_sample(const char* path, int* nbgrains, double** r, double** x1, double** x2);
void lbmdem_free_host(void* p);

/* Allocation + initial state, replacing main.c:1802-1834,1858-1861: f = w[q] (init_density,
 * main.c:716-724), grains at rest with m, It from r (main.c:624-635), rLB, and the initial obstacle
 * map (init_obst, main.c:663-711). r, x1, x2 in metres, nbgrains entries each. */
int lbmdem_create(const lbmdem_config* cfg, const double* r, const double* x1, const double* x2,
                  lbmdem_handle** out);
int lbmdem_destroy(lbmdem_handle* h);

/* ---- the hot path --------------------------------------------------------------------------- */

/* One fluid step = main.c:1711-1713,1717: reinit_obst_density (966-986), obst_construction
 * (991-1065), collision_streaming (1071-1243), forces_fluid (1285-1333). */
int lbmdem_lbm_step(lbmdem_handle* h);
/* The same, phase by phase (lbm_step == obst_construction; collide_stream; forces_fluid).
 * reinit_obst_density is folded into collide_stream: it needs the *previous* obstacle map, which
 * the library keeps. */
int lbmdem_obst_construction(lbmdem_handle* h); /* main.c:991-1065 (obst only; act, delta are recomputed on the fly) */
int lbmdem_collide_stream(lbmdem_handle* h);    /* main.c:966-986 + 1071-1243 */
int lbmdem_forces_fluid(lbmdem_handle* h);      /* main.c:1285-1333 */

/* Diagnostic for the parity force kernel: the fused collide_stream kernel leaves every bounce-back link's
 * momentum-exchange sum (main.c:1313-1316) in a per-grain table, and forces_fluid replays them in the reference's
 * order without touching the lattice; grains with a link that ends in a non-fluid node (another grain, a
 * lattice-edge wall), with overlapping discs, or cut by a strip boundary are gathered from obst and f instead --
 * same bits either way. Returns how many grains of the LAST forces_fluid call took each route (from_table = 0
 * when the table did not describe the current lattice and every grain was gathered). Synchronises. */
int lbmdem_force_stats(lbmdem_handle* h, int* from_table, int* gathered);
/* Which size-dependent fast paths are active on this handle: info4[0] link-sum table (needs < 2^18 grains, reduced radius
 * < ~20 nodes, reductionR < 1), info4[1] its slots per direction, info4[2] the lowest-cover record that keeps `act` exact
 * where three or more reduced discs overlap (< 2^20 grains; else the two-disc rule), info4[3] the marching fused kernel. */
int lbmdem_path_info(lbmdem_handle* h, int* info4);
/* How the fused kernel's launch over this handle's rows is cut into work items (windows of 60 columns -- MARCH_WW -- x segments of rows):
 * info12 = {levels, rows per XCD band, rows per interleaved chunk, segment rows of level 0..3, band rows cut at level 0..3,
 * work items in all}. levels == 0: uniform segments of info12[3] rows (short row ranges: strips, small lattices); else the
 * tapered order (long segments first, short ones last) of DESIGN.md section 4. Host-side arithmetic only. */
int lbmdem_fused_work_order(lbmdem_handle* h, int* info12);

/* initVerlet + VerletWall, main.c:1519-1594 (same pair set; uniform grid + radix sort instead of
 * the O(N^2) scan). Also moves the right/top DEM walls as VerletWall does (main.c:1555-1561). A wall that takes another value
 * here invalidates what was computed with the walls as they were: the Voronoi readers and the cluster readers are refused until
 * their next compute, the contact export until the next table sub-step; walls that keep their values leave them readable. */
int lbmdem_verlet_rebuild(lbmdem_handle* h);

/* One DEM sub-step = main.c:1733-1764: drift + half kick, acceleration_grains (1336-1516, film
 * law when nbsteps % stepFilm == 0), second half kick, nbsteps++. */
int lbmdem_dem_substep(lbmdem_handle* h);

/* n x renderScene() (main.c:1697-1765) with the reference's cadences: a fluid step when
 * nbsteps % npDEM == 0, a Verlet rebuild when nbsteps % updateVerlet == 0, then a DEM sub-step.
 * Device-resident; returns without synchronising. */
int lbmdem_run(lbmdem_handle* h, long n_dem_steps);
/* The same without the fluid steps: n x (Verlet rebuild when due; DEM sub-step). For drivers that run the
 * fluid step themselves (strip decomposition: halo exchange and force combine sit between its phases). */
int lbmdem_run_dem(lbmdem_handle* h, long n_dem_steps);

/* The reference's whole main loop, `do { renderScene(); ... } while (nbsteps * dt <= duration)` (main.c:1879-1890), with
 * everything that hangs on the step counter besides the step itself. lbmdem_scene_schedule is the single place these
 * cadences live. With `s` the counter BEFORE a sub-step and s' = s + 1 after it, a sub-step's events in the loop's order:
 *   LBMDEM_SCENE_CONSOLE_DENSITY  fluid && s % npDEM == 0 && s % 400 == 0 (main.c:1715): the fluid step, then check_density's
 *                                 line, then the list rebuild if due, then the sub-step                      (step = s)
 *   LBMDEM_SCENE_VTK              s' % stepFilm == 0 (main.c:1767-1772): write_vtk when `fluid`, with nfile; nFile++ either way
 *   LBMDEM_SCENE_DEM              s' % 4000 == 0 (main.c:1773-1776): write_DEM, write_forces with the NEW nFile
 *   LBMDEM_SCENE_STEPS_LINE       s' % updateVerlet == 0 (main.c:1884-1889): the "steps ... KE ... Time" line with the
 *                                 energies of the last write_DEM
 *   LBMDEM_SCENE_STOP             the first s' with (double)s' * cfg->dt > duration -- found with that predicate itself, as the
 *                                 loop evaluates it (main.c:1890), not by a division; a do-while: a run that starts beyond it
 *                                 still makes one sub-step. duration < 0: no stop. The list ends with this event.
 * (step = s' for the last four; nfile = the frame counter the event uses, nFile = nbsteps0 / stepFilm at the start as
 * main.c:147.) Host only, no handle, no device: the events of n calls of renderScene() starting at counter nbsteps0. At most
 * `cap` of them are written to `out`; *count receives how many there are (cap = 0 to size). */
#define LBMDEM_SCENE_CONSOLE_DENSITY 0
#define LBMDEM_SCENE_VTK 1
#define LBMDEM_SCENE_DEM 2
#define LBMDEM_SCENE_STEPS_LINE 3
#define LBMDEM_SCENE_STOP 4
typedef struct lbmdem_scene_event { int kind; int nfile; long step; } lbmdem_scene_event;
int lbmdem_scene_schedule(const lbmdem_config* cfg, long nbsteps0, long n, double duration, int fluid,
                          lbmdem_scene_event* out, long cap, long* count);
typedef struct lbmdem_comm lbmdem_comm;   /* the RCCL transport of a strip decomposition (lbmdem_comm_*, below) */
/* The loop itself: n x renderScene() from the handle's step counter, or fewer when the stop condition ends it, with the
 * console lines and files of that schedule. The sub-steps between two events go to the run loop in ONE call (lbmdem_run;
 * lbmdem_run_dem when !fluid; lbmdem_comm_run with a communicator), so that runs of ordinary sub-steps are single launches
 * whose tail rasterises for the next fluid step; a sub-step whose events all follow it is the last of such a stretch. At an
 * event: CONSOLE_DENSITY = lbmdem_move_walls on a vibrating handle, lbmdem_lbm_step (lbmdem_comm_lbm_step), the serial
 * chain of lbmdem_total_density_serial (through the ranks in x order), the line, lbmdem_verlet_rebuild if due,
 * lbmdem_dem_substep; VTK = lbmdem_write_vtk (lbmdem_comm_write_vtk: collective, rank 0 writes); DEM = lbmdem_write_dem +
 * lbmdem_write_forces on rank 0. The writers and the phase calls settle the handle first like every entry point outside
 * lbmdem_run / lbmdem_run_dem: a launch of the multi-sub-step kernel that gave up is undone and its sub-steps are repeated
 * before anything is written or printed. The state after the call is that of lbmdem_run called steps_done times with 1.
 * Lines: "Iteration Number %ld, Total density in the system %f\n" (main.c:1259) and "steps %li steps %le KE %le PE %le SE
 * %le WF %le INCE %le SLIP %le RW %le Time %s \n" with asctime (main.c:1885-1889), on rank 0 only, each passed whole to
 * `say`. The energies of the last write_DEM stay in the handle: a second call prints what the first one's left. The header
 * line of stats.data is the caller's (the reference writes it in main(), main.c:1867-1877). With a communicator every rank
 * makes the same call (same n, dir, duration). The single-precision library has no write_DEM / write_forces: there a DEM
 * event with a directory fails with LBMDEM_EINVAL, by those writers' own refusal (dir = NULL needs none). */
typedef struct lbmdem_scene {
  const char* dir;      /* files go here; NULL = write no files (events still happen: nFile still advances) */
  int fluid;            /* 1: the reference as shipped; 0: without _FLUIDE_ (main.c:16): no fluid step, no density line, no VTK */
  double duration;      /* main.c:47; < 0: run all n */
  void (*say)(void* user, const char* line);   /* console lines, one call per line; NULL = stdout */
  void* user;
} lbmdem_scene;
typedef struct lbmdem_scene_result {
  long steps_done;      /* sub-steps this call made */
  int nfile;            /* the frame counter after them */
  int stopped;          /* 1: the stop condition ended the loop */
  double energies8[8];  /* KE, PE, SE, IFR, WF, INCE, TSLIP, TRW of the last write_DEM (lbmdem_write_dem) */
  double last_density;  /* the last check_density sum of this call (0 when there was none) */
} lbmdem_scene_result;
int lbmdem_run_scene(lbmdem_handle* h, lbmdem_comm* comm /* NULL: one domain */, long n, const lbmdem_scene* sc,
                     lbmdem_scene_result* res /* may be NULL */);

/* Device-side probes: the field diagnostics the reference has routines for but never calls, recorded
 * on the device every `every`-th fluid step without the host taking part, and fetched afterwards. A sample is taken right
 * after forces_fluid of a fluid step (main.c:1710-1718), before that renderScene's list rebuild and DEM sub-step: it sees f
 * after collision_streaming, obst as obst_construction built it in this step, the grains as the sub-step before left them.
 * Fluid steps 0, every, 2 every, ... counted from lbmdem_probe_enable are sampled -- in lbmdem_lbm_step, lbmdem_run,
 * lbmdem_run_scene, and by lbmdem_forces_fluid when the phases are called one by one. One record, all doubles, in this order
 * (reference arithmetic, same association):
 *   step, time, clock       the counter s, s * dt, and a vibrating handle's clock t (else 0)
 *   pressure_row[lx]        row y = pressure_row (the reference uses 2) of write_densities' pressure_base file, main.c:524-539:
 *                           P = 0.; P += f[x][y][i] for i = 0..8; (1./3.) * rho_moy * (P - 1.) where obst < 0, else 0.0
 *   velocity_y              the row of velocity_profile, y = (int)((g[0].x2 - Mby) / dx) (main.c:1658), clamped into
 *                           [0, ly-1] (the reference does not clamp) ...
 *   velocity_row[lx]        ... and its values, main.c:1660-1672: g[obst].v2 / c on a grain, else u_y / d_loc of the node
 *   point_pressure[npoints] `pressures` (main.c:1685-1691) at the given nodes: (f0 + ... + f8 - rho_moy) * c_squ where
 *                           obst == -1, else 0.
 *   xgrainmax, height       max (x1 + r), max (x2 + r) over the grains (write_DEM, main.c:400-405); 0 if none is positive
 * lbmdem_probe_layout gives where each of these six starts in a record (-1: switched off). The ring holds `capacity`
 * records; when it is full further samples are dropped and counted, never overwritten and never waited for, until
 * lbmdem_probe_read has emptied it. lbmdem_probe_read settles and synchronises the handle, copies the records (oldest
 * first), reports how many samples were dropped since the last read, and empties the ring; out = NULL only reports the
 * counts; a buffer of fewer than *count records is refused. Off by default: then nothing is launched or allocated.
 * LBMDEM_EINVAL: on a strip of a decomposition or with distributed grains (and lbmdem_dist_enable on a probing handle),
 * in the single-precision library, for a point or pressure_row outside the lattice, for more than
 * LBMDEM_PROBE_MAX_POINTS points, and when capacity x record size exceeds 1 GiB. Checkpoints do not carry probes: a loaded
 * handle has none. */
#define LBMDEM_PROBE_MAX_POINTS 64
typedef struct lbmdem_probe_config {
  int every;          /* sample every k-th fluid step, k >= 1 */
  int capacity;       /* records the device ring holds */
  int pressure_row;   /* y of the pressure profile (the reference uses 2); < 0: off */
  int velocity_row;   /* 1: the profile of main.c:1647-1676; 0: off */
  int npoints;        /* 0..64 */
  const int* points;  /* npoints x (x, y) */
  int grain_extent;   /* 1: xgrainmax, height */
} lbmdem_probe_config;
int lbmdem_probe_enable(lbmdem_handle* h, const lbmdem_probe_config* pc);   /* allocates; replaces an earlier set-up */
int lbmdem_probe_disable(lbmdem_handle* h);
long lbmdem_probe_record_doubles(lbmdem_handle* h);                         /* length of one record */
int lbmdem_probe_layout(lbmdem_handle* h, long* offsets6);
int lbmdem_probe_read(lbmdem_handle* h, double* out, long cap_records, long* count, long* dropped);

/* EXTENSION, not in the reference as it runs: a lid. The reference's top-plate copies carry commented-out moving-wall
 * terms (main.c:1129-1130: f[x][ly-1][3] = f[x-1][ly-2][7]; //-uw_h/6;  f[x][ly-1][5] = f[x+1][ly-2][1]; //+uw_h/6;
 * `uw_h` is not even declared). lbmdem_set_lid enables exactly those two terms with uw_h in lattice units (0 = off, the
 * default) -- BASELINE.json configs[1], a lid-driven cavity. Checked against the CPU oracle carrying the same terms. */
int lbmdem_set_lid(lbmdem_handle* h, double uw_h);

/* The reference's shaken box, `vib = 1` (main.c:162-165). Every renderScene() then starts by advancing the clock t by dt
 * and moving the left wall Mgx and the right wall Mdx each by amp times the sine of freq times the new t (main.c:1700-1705),
 * and the fluid step (rasterisation main.c:1009, wall velocity of reinit_obst_density and the IBB main.c:974-980,1172-1216,
 * torque arm main.c:1296,1320), the Verlet rebuild and the DEM sub-step (the top wall's amp*freq*cos(freq*t), main.c:855)
 * all use the moved walls. As written there: the rebuild's VerletWall resets Mdx (main.c:1555-1561), discarding its offset,
 * while Mgx keeps moving away; the lattice-edge walls of the fluid and dx do not move. Same bits as the reference.
 * lbmdem_set_vibration(h, 1) switches it on (off by default) with freq, amp of cfg.phys and the clock and walls where they
 * are (cfg.phys.t, cfg.Mgx, cfg.Mdx at create, or as a checkpoint saved them); 0 stops the walls where they are. The walls
 * move in lbmdem_run and lbmdem_run_dem, once per sub-step, before its fluid step; the separate phases use them as they are.
 * A checkpoint of a vibrating handle restarts vibrating.
 * Not available (LBMDEM_EINVAL): on a strip of a decomposition or with distributed grains (lbmdem_dist_enable, the host
 * driver's --gpus N), and in the single-precision library (liblbmdem_hip_sp.so), which has no checker for this mode. */
int lbmdem_set_vibration(lbmdem_handle* h, int on);
int lbmdem_vibration(lbmdem_handle* h);   /* 1 when on, 0 when off */
/* renderScene's first statement alone (main.c:1700-1705), for callers that run the phases themselves (lbmdem_lbm_step,
 * lbmdem_verlet_rebuild, lbmdem_dem_substep) instead of lbmdem_run: once per sub-step, before its fluid step. A wall that
 * changes value (amp != 0) invalidates what was computed with the walls as they were: the Voronoi readers are refused until the
 * next lbmdem_voronoi_compute, the contact export, lbmdem_cluster_compute and the cluster readers until the next table sub-step. */
int lbmdem_move_walls(lbmdem_handle* h);
/* walls5 = t, Mgx, Mdx, Mby, Mhy as the next sub-step finds them (before its renderScene moves them) */
int lbmdem_get_walls(lbmdem_handle* h, double* walls5);
/* Host only: the walls the reference uses on sub-steps nbsteps0 .. nbsteps0 + n - 1 of a vibrating run that has cfg's clock
 * and walls before sub-step nbsteps0 -- out[4 k .. 4 k + 3] = t, Mgx, Mdx and the top wall's amp*freq*cos(freq*t), in the
 * order of renderScene (the move, then the rebuild's reset of Mdx when nbsteps % updateVerlet == 0, with the dtt switch). */
int lbmdem_vibration_schedule(const lbmdem_config* cfg, long nbsteps0, long n, double* out);

/* hydrodynamic-force summation: 0 = parity (the reference's order of additions, bit-exact); 1 = fast (the same
 * addends reduced across the lanes of a wavefront: differs in the last bits; same speed as parity since round 2,
 * kept for callers that do not need the reference's bits). Default 0. */
int lbmdem_set_force_mode(lbmdem_handle* h, int mode);

/* lbmdem_run / lbmdem_run_dem / lbmdem_comm_run hand every run of ordinary sub-steps (renderScene calls between which
 * nothing else happens: no fluid step main.c:1710, no list rebuild main.c:1721, regular contact law main.c:1427-1451, no
 * write_DEM diagnostics main.c:1773) to ONE kernel launch of at most `max_substeps` sub-steps: the tiles of grains hand
 * their drifted state (main.c:1748-1753) to their partners' tiles through tagged cache-line records instead of kernel
 * boundaries. Same bits as lbmdem_dem_substep called that many times. < 2: one launch per sub-step. Default 128. The
 * library falls back to one launch per sub-step by itself where the tiles of a packing cannot all be resident at once. */
/* obst_construction (main.c:991-1065) clears the map and paints every disc again; between two fluid steps a disc moves by
 * a fraction of a node. on = 1: the rasteriser compares every disc's footprint at the centre it was last painted at in that
 * map buffer with its footprint now and writes only the nodes whose owner changes (no reset of the canvas; a disc that has
 * not moved far enough for any node to change sides is skipped altogether; needs the pair list: falls back to clear +
 * repaint by itself before the first list, after an upload of positions, with distributed grains, and while a grain has
 * outrun the list). Same maps bit for bit. on = 0 (default): clear + repaint every step -- on an agitated packing the update
 * is no faster (the rasteriser is bound by its per-grain set-up, not by its stores: 36 against 30 + 4 us at 50 000 grains), on
 * one at rest it is (16 us). lbmdem_obst_stats: how often each ran. */
int lbmdem_set_obst_update(lbmdem_handle* h, int on);
int lbmdem_obst_stats(lbmdem_handle* h, long* updates, long* repaints);
/* reinit_obst_density (main.c:966-986) needs the PREVIOUS owner of a node, i.e. the map of the step before, at the few
 * thousand nodes that changed hands. mode 1 (default): a rasterisation in place by the end of a run of sub-steps also
 * leaves one bit per lattice row and 64-column window of the fused kernel -- "the two maps differ here" -- and the fused
 * kernel of a whole single-domain step reads the second map only in those rows (4 of its 152 bytes per node otherwise).
 * 0: both maps are read everywhere. 2: as 1, and every use is checked (tests): the bits against the two maps, and the
 * populations against a second launch that reads both maps everywhere (into a scratch lattice).
 * lbmdem_change_mask_stats: fused launches that used the bits; what mode 2 found wrong -- low 32 bits: (row, window)
 * pairs whose bit was clear over differing maps, high 32 bits: populations that differed -- must be 0. */
int lbmdem_set_change_mask(lbmdem_handle* h, int mode);
int lbmdem_change_mask_stats(lbmdem_handle* h, long* used, long* hidden);

int lbmdem_set_dem_chain(lbmdem_handle* h, int max_substeps);
/* what that path has done so far: launches, sub-steps they covered, the workgroups ("tile slots": 64 grains each) one
 * launch needs resident at once, and how many the census found resident (-1: not taken yet, 0: they do not fit) */
int lbmdem_dem_chain_stats(lbmdem_handle* h, long* launches, long* substeps, int* tile_slots, int* resident);
/* A run that ends where a fluid step begins also rasterises the reduced discs (obst_construction's paint, main.c:1009-1032)
 * at the positions it ends with -- they and those of all partners are in the tiles' on-chip memory then: the next
 * lbmdem_obst_construction has nothing left to launch. lbmdem_dem_chain_paints: how often that happened.
 * lbmdem_set_dem_chain(h, -1) switches only this off (A/B). Same maps bit for bit. */
int lbmdem_dem_chain_paints(lbmdem_handle* h, long* paints);
/* A launch of that kernel needs all its workgroups on the GPU at once, which HIP does not promise (another process, a CU
 * mask): every wait in it is bounded, and a launch that gives up cannot end a run -- the reference's loop (main.c:1733-1763)
 * cannot fail either. It raises a stop word that every kernel queued behind it looks at first, so the device keeps the
 * state the launch started from; the next call that is not lbmdem_run / lbmdem_run_dem (or the 256th launch since) drains
 * the stream, takes the handle back to that launch, switches the multi-sub-step kernel off for the handle and repeats the
 * sub-steps since, one launch each: the same bits. lbmdem_dem_chain_recoveries: how often that has happened (0 on a GPU of
 * its own). Distributed handles (lbmdem_dist_*) report the failure instead: a rank cannot go back alone.
 * The setters are such calls too -- lbmdem_set_lid, lbmdem_set_force_mode, lbmdem_set_nbsteps, lbmdem_set_obst_update,
 * lbmdem_set_change_mask, lbmdem_set_diagnostics, lbmdem_set_dem_chain, lbmdem_set_vibration: a setting takes effect at its
 * call and never on sub-steps asked for before it, whether or not a launch among them had to be repeated.
 * lbmdem_set_dem_chain(h, k) keeps the caller's k even when its own drain finds such a launch (the switch-off comes
 * first); after a recovery found by any other call the kernel stays off until lbmdem_set_dem_chain is called again.
 * A list rebuild queued behind a launch that gave up leaves the pair list alone, on a handle loaded from a checkpoint too. */
int lbmdem_dem_chain_recoveries(lbmdem_handle* h, long* count);
/* The grains of that kernel's workgroups ("tiles" of 64). mode 1 (default): consecutive stretches along a space-filling
 * curve over the positions at lbmdem_create (or at this call) -- compact patches of the packing whatever the numbering of the
 * grains, so that a tile's partners outside itself are the patch's rim: the reference's own bin/50000.data, whose numbering
 * is not coherent in space, then runs at the pace of a row-numbered packing. 0: by index (tile t = grains 64 t .. 64 t + 63).
 * Only speed depends on it: a grain's sums keep the reference's order (partners ascending by index, main.c:1427-1451). */
int lbmdem_set_dem_tiles(lbmdem_handle* h, int mode);

/* ---- state in / out (host layout) ------------------------------------------------------------ */

int lbmdem_upload_f(lbmdem_handle* h, const double* f_aos);   /* [lx][ly][9]; rows of the local strip+halo are read */
int lbmdem_download_f(lbmdem_handle* h, double* f_aos);       /* [lx][ly][9]; only the OWNED rows are written */
int lbmdem_download_obst(lbmdem_handle* h, int* obst);        /* [lx][ly]; owned rows */
int lbmdem_download_macro(lbmdem_handle* h, double* rho, double* ux, double* uy); /* [lx][ly] each; owned rows; sums of f, f*ex, f*ey as write_vtk forms them (main.c:315-319) */
int lbmdem_total_density(lbmdem_handle* h, double* sum);      /* sum of f over the owned rows, tree order (fast; last bits differ from the reference's serial sum) */
/* check_density / final_density (main.c:1249-1273) with the reference's own bits: the serial chain sum = sum + f[x][y][q]
 * (x outer, y, q inner) continued from `sum_in` over the owned rows -- 0 for one domain; a strip passes its result to the
 * next strip. Computed on the device as integer quanta per lattice row wherever the running sum stays in one binade
 * (exact), rows where it does not are replayed element by element; `rows_replayed` (may be null) counts those. */
int lbmdem_total_density_serial(lbmdem_handle* h, double sum_in, double* sum_out, int* rows_replayed);
/* kinematics table, 9 doubles per grain: x1 x2 x3 v1 v2 v3 a1 a2 a3 */
int lbmdem_upload_kinematics(lbmdem_handle* h, const double* k9);
int lbmdem_download_kinematics(lbmdem_handle* h, double* k9);
int lbmdem_download_fhf(lbmdem_handle* h, double* fhf3);      /* interleaved fhf1,fhf2,fhf3 (main.c:180) */
/* Verlet lists in the reference's form: cumul[n] (main.c:150,1539), neighbours (j > i, ascending),
 * wall membership flags per grain (bit0 B, bit1 T, bit2 L, bit3 R; main.c:1563-1593).
 * `cap` = capacity of neighbours[]; *npairs receives the pair count (call with cap = 0 to size). */
int lbmdem_download_verlet(lbmdem_handle* h, int* cumul, int* neighbours, int cap, int* npairs,
                           int* wallflags);
/* grain pressure g.p of the last DEM sub-step (main.c:187: sum of the normal contact forces) */
int lbmdem_download_grain_pressure(lbmdem_handle* h, double* p);
/* The five float32 fields write_vtk builds (main.c:272-323): grain_pressure[ly][lx], grain_velocity
 * [ly][lx][3], grain_acceleration[ly][lx][3], fluid_pressure[ly][lx], fluid_velocity[ly][lx][3] (owned
 * rows: lx = x_end - x_begin); computed on the device with the reference's float accumulation. */
int lbmdem_download_vtk_fields(lbmdem_handle* h, float* grain_pressure, float* grain_velocity,
                               float* grain_acceleration, float* fluid_pressure, float* fluid_velocity);
/* write_vtk (main.c:237-338 -> visit_writer.c write_rectilinear_mesh, binary): writes the five files
 * <dir>/{grain_pressure,grain_velocity,grain_acceleration,fluid_pressure,fluid_velocity}_NNNNNN.vtk,
 * byte-identical to the reference's. Single-domain handles only. */
int lbmdem_write_vtk(lbmdem_handle* h, const char* dir, int nfile);
/* The same five files, written in the background while the run goes on. lbmdem_set_async_output(h, frames), frames in
 * 1..LBMDEM_ASYNC_MAX_FRAMES, sets up that many frame slots (device staging + pinned host memory of lbmdem_vtk_image_bytes
 * each), a copy stream and one writer thread; 0 drains, joins and frees them (the default: nothing is allocated, no thread
 * exists). lbmdem_write_vtk_async settles the handle like every writer, takes a free slot -- when none is free it waits for
 * the writer: a frame is never dropped --, launches ONE kernel on the handle's stream that leaves the frame in the slot as the
 * files hold it (the five payloads back to back, big-endian float32, 44 bytes per node: the "image"), queues the copy to
 * pinned memory on the copy stream behind an event, hands the slot to the writer and returns without synchronising: the
 * step stream is held for that kernel only, and what is stepped afterwards does not reach the frame. The files are those of
 * lbmdem_write_vtk byte for byte. The writer reports nothing itself: its first failure (a directory that does not exist,
 * a full disk) is returned, with its text as lbmdem_last_error, by the next lbmdem_write_vtk_async, lbmdem_output_drain or
 * lbmdem_run_scene on the handle and is then forgotten (lbmdem_destroy drops it); the handle stays usable.
 * lbmdem_output_drain returns when every queued frame is on disk and closed. On a handle with async output on,
 * lbmdem_run_scene (comm = NULL) hands its VTK events to lbmdem_write_vtk_async and drains before it returns: its files exist
 * when it returns, as before. write_DEM / write_forces stay synchronous (lbmdem_set_async_dem, below, is their switch). lbmdem_output_stats -- counts4: frames queued,
 * written, failed, calls that had to wait for a slot; ms4: the caller waiting for a slot, the writer waiting for copies,
 * the writer in file I/O, the caller in lbmdem_output_drain (all 0 while off).
 * LBMDEM_EINVAL: frames outside 0..4, lbmdem_write_vtk_async while off, a strip of a decomposition or distributed grains
 * (and lbmdem_dist_enable on a handle with async output on). LBMDEM_ENOMEM: the slots cannot be had (then the feature is
 * off). Vibrating and probing handles and the single-precision library have it. Checkpoints do not carry the setting. */
#define LBMDEM_ASYNC_MAX_FRAMES 4
int lbmdem_set_async_output(lbmdem_handle* h, int frames);          /* 0: off (default) */
int lbmdem_write_vtk_async(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_output_drain(lbmdem_handle* h);                          /* LBMDEM_OK at once while off */
int lbmdem_output_stats(lbmdem_handle* h, long* counts4, double* ms4);
/* Host only, no handle, no device: the size of an image (44 * lx * ly), and the five files from one -- the header of
 * lbmdem_write_vtk's files, then each payload in one write straight from the image. */
size_t lbmdem_vtk_image_bytes(int lx, int ly);
int lbmdem_write_vtk_image(const char* dir, int nfile, int lx, int ly, const void* image_be);
/* the image of the present state into a caller's host buffer of lbmdem_vtk_image_bytes (the snapshot kernel alone,
 * synchronously; whole-lattice handles, async output on or off) */
int lbmdem_download_vtk_image(lbmdem_handle* h, void* image_be);
/* Contact diagnostics of the last DEM sub-step (what write_DEM prints, main.c:340-438). They are produced
 * in the sub-step that brings the step counter to a multiple of stepStrob = 4000 (main.c:142,1773), or in
 * every sub-step after lbmdem_set_diagnostics(h, 1). Table: 30 doubles per grain in the reference's struct
 * order (main.c:182-197): x1 x2 x3 v1 v2 v3 a1 a2 a3 r m mw It p s f1 f2 ifm fm fr ifr M11 M12 M21 M22 ice
 * slip rw z zz. fr, ice, slip, rw read "previous contact" carries that thread through the reference's serial
 * contact loop and from sub-step to sub-step (pft, pff, pf, ic: main.c:130-131); the library replays them in
 * the reference's order in the table sub-steps; the carries such a sub-step starts from are those of the last
 * contact of each kind however many sub-steps ago (every ordinary sub-step records its last contacts per tile of
 * grains; single-domain handles). */
int lbmdem_set_diagnostics(lbmdem_handle* h, int always);
int lbmdem_download_grain_table(lbmdem_handle* h, double* table30);
/* write_DEM (main.c:340-438): <dir>/DEM%06d.dat and one line appended to <dir>/stats.data; energies8 (may be
 * NULL) receives energie_cin, energy_p, SE, IFR, WF, INCE, TSLIP, TRW for the console line of main.c:1885-1889. */
int lbmdem_write_dem(lbmdem_handle* h, const char* dir, int nfile, double* energies8);
/* write_forces (main.c:440-478): <dir>/DEM%06d.ps, a PostScript picture of the grains (grey level from g.fm)
 * and one line per overlapping pair, in the reference's order (i outer, j inner, both directions). The
 * reference reads g[nbgrains], one element past its array, and its three "%%%Word" header formats are
 * undefined conversions; this writer emits the nbgrains real grains and the headers the format strings
 * evidently mean. Every other line is character-identical to the reference's file. The pair search is a
 * host-side uniform grid (same pairs as the reference's O(N^2) loop). */
int lbmdem_write_forces(lbmdem_handle* h, const char* dir, int nfile);
/* The boundary-link export: the two arrays of obst_construction (main.c:991-1065) that the library never stores -- act[x][y],
 * which solid nodes take part in the bounce-back, and delta[x][y][q], the wall distance of every link -- derived on the device
 * from the obstacle map with the device functions the fluid step itself uses, and obst_writing (main.c:1601-1641), the
 * reference's dump of them: <dir>/obst_LB.dat, <dir>/active_nodes.dat, <dir>/links.dat.
 * Which geometry: the MOST RECENT RASTERISATION -- the map the library painted last, together with the centres it was painted
 * from. After lbmdem_create, lbmdem_obst_construction, lbmdem_lbm_step or a fluid step inside a run that is the map
 * lbmdem_download_obst returns. After a run whose last sub-steps have already rasterised the discs for the coming fluid step
 * (lbmdem_dem_chain_paints) it is that new map, which lbmdem_download_obst does not show yet: lbmdem_download_geometry_obst
 * hands back the map the other three calls describe, whichever it is. The export launches no rasterisation and changes nothing
 * a later step reads: a run with exports in between is bit-equal to the run without them.
 * A link is an EFFECTIVE link: a (node P, direction q) that the reference's bounce-back loop (main.c:1154-1222) takes into its
 * interpolation branch -- P an interior node of a grain (obst[P] != -1, != nbgrains), act[P] == 1, obst[P + e_q] == -1. Its
 * delta is bit for bit the reference's delta[P][q] (the owner of P is the last grain to write that entry). The reference's
 * delta array can hold further non-zero entries that its loop never reads: left by a lower-index disc at a node, or towards a
 * neighbour, that a higher-index disc painted afterwards. These STALE entries are no links and are not exported; they exist
 * only where two reduced discs overlap or sit on adjacent nodes -- in every other packing the links are exactly the
 * reference's delta != 0 entries and links.dat is the reference's file character for character.
 * Links come in the file's order: y outer, x inner, q = 1..8. A link whose delta is exactly zero -- which the reference's file
 * leaves out (its `!= 0` test, main.c:1634) -- stays in the list with q NEGATED; the formatter skips it.
 *   lbmdem_geometry_stats          counts6 = solid interior nodes, active solid nodes, effective links (zero deltas included),
 *                                  links with 0 < delta < 1/2, links with delta >= 1/2, solid -> solid slots at active nodes
 *                                  (the w[q] resets of main.c:1161, 1192). The counting pass alone.
 *   lbmdem_download_act            [lx][ly], the reference's values: 1 on interior fluid, 0 on the lattice-edge rows and columns
 *                                  (init_obst, main.c:675-683), 0 or 1 on grains
 *   lbmdem_download_links          cap = 0 (out may be NULL) only reports *count; a buffer of fewer than *count records is refused
 *   lbmdem_write_obst_files        host only, no handle, no device: the one formatter -- "%d " per node and "\n" per y for the two
 *                                  maps, "%d  %d  %d  %f\n" per link. Unlike the reference it checks fopen.
 * LBMDEM_EINVAL: a strip of a decomposition or distributed grains; the single-precision library; null buffers; a handle whose
 * last rasterisation was given up or replaced (the grains moved on by sub-steps or an upload after a run had painted for a
 * fluid step that never came; a loaded checkpoint before its first fluid step). Vibrating and probing handles have the export;
 * a checkpoint carries nothing of it. */
typedef struct lbmdem_link { int x, y, q, grain; double delta; } lbmdem_link;
int lbmdem_geometry_stats(lbmdem_handle* h, long* counts6);
int lbmdem_download_act(lbmdem_handle* h, int* act);
int lbmdem_download_links(lbmdem_handle* h, lbmdem_link* out, long cap, long* count);
int lbmdem_download_geometry_obst(lbmdem_handle* h, int* obst);
int lbmdem_write_obst(lbmdem_handle* h, const char* dir);
int lbmdem_write_obst_files(const char* dir, int lx, int ly, const int* obst, const int* act, const lbmdem_link* links, long n);
/* The contact network export: the reference declares `struct contact { int i, j; real nx, ny; real fn, ft; }` ("Luding Friction
 * Model", main.c:167-174) and never fills it, and write_forces was meant to draw every contact with the line width of its normal
 * force (the term is commented out, main.c:469). The library keeps only per-grain sums; the per-contact values exist in the
 * registers of the sub-step kernels. The export re-derives them on the device, with the device functions the sub-step itself
 * uses, from the state the sub-step STARTED from, which the other half of the kinematics ping-pong still holds.
 * Which contacts: those of the LAST sub-step, when it was a table sub-step (every 4000th, or every one after
 * lbmdem_set_diagnostics(h, 1)) -- the condition of lbmdem_download_grain_table -- evaluated with that sub-step's pair list, wall
 * flags, contact law (regular or film) and parameters (walls and clock as they stood when it was launched). Any other sub-step
 * or run of sub-steps, lbmdem_verlet_rebuild, lbmdem_upload_kinematics, lbmdem_dist_enable and a loaded checkpoint end that:
 * every call below then returns LBMDEM_EINVAL and names lbmdem_set_diagnostics.
 * Grain-grain records: one per pair i < j of the list with dn < 0 (main.c:744), i ascending, j ascending -- the reference's loop
 * order. dn, nx = xn, ny = yn of main.c:739-753 (the normal points from j to i), fn and ft the law's variables after the clamps
 * (main.c:761-771; main.c:1380-1390 on a film step), bit for bit what the sub-step used. A pair with fn == 0 is a record.
 * Wall records follow all pair records: grain ascending, wall B, T, L, R within a grain. j = the wall code, dn the law's gap,
 * (nx, ny) the inward wall normal (0,1), (0,-1), (1,0), (-1,0), fn and ft the reference's variables of those names in
 * force_WallB/T/L/R when the function returns (top and right: fn <= 0; the right wall's ft comes from the unclamped fn).
 *   lbmdem_contact_stats           counts6 = candidate pairs (list entries i < j), touching pairs, touching pairs that took the
 *                                  Coulomb clamp branch, touching pairs with fn == 0, wall contacts, grains with at least one
 *                                  record. The counting pass alone.
 *   lbmdem_download_contacts       cap = 0 (out may be NULL) only reports *count; a buffer of fewer than *count records is refused
 *                                  with *count set; synchronises; changes nothing a later step reads
 *   lbmdem_write_contacts_files    host only, no handle, no device: <dir>/contacts%.6i.dat -- "# i j dn nx ny fn ft", then
 *                                  "%d %d %le %le %le %le %le\n" per record -- and <dir>/DEM%.6i_chains.ps -- header and one arc
 *                                  per grain as lbmdem_write_forces prints them (fm: the grey level), then per grain-grain record
 *                                  with fn > 0 the four lines of main.c:469-473 with fn as the line width: one group per contact.
 *                                  It checks fopen.
 *   lbmdem_write_contacts          the download, then that formatter with r, x1, x2, fm of lbmdem_download_grain_table
 *   lbmdem_set_contacts_output     on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_contacts at every DEM event, right
 *                                  behind write_DEM / write_forces (queued first where tables go to the background), with the same
 *                                  nFile. Off by default; a checkpoint does not carry it.
 * LBMDEM_EINVAL: a strip of a decomposition or distributed grains (and lbmdem_dist_enable with the setting on); the
 * single-precision library (the host-only formatter exists there too); null buffers; a directory that cannot be written.
 * Vibrating and probing handles have the export. A wall that lbmdem_move_walls gives another value invalidates the records: the
 * three calls are refused (LBMDEM_EINVAL, "a wall has been moved since the last table sub-step") until the next table sub-step,
 * since the handle's walls are no longer the ones that sub-step saw. lbmdem_verlet_rebuild invalidates them whether a wall moves
 * or not (the list that sub-step walked is gone), with the sentence of a handle without a table sub-step. A fluid step alone
 * (lbmdem_lbm_step), lbmdem_upload_f, the coarse-grained and the flow fields move no grain and no wall: the contact export, the
 * clusters, the structure and the Voronoi readers go on answering (a fluid step raises no sub-step count; the coarse and the flow
 * fields, which read the populations, change with it). Every call counts the records anew; one that has room for all of them
 * (lbmdem_write_contacts, and lbmdem_cluster_compute for itself) also emits them into the export's own buffer: the same records, in
 * the same order, as often as it is asked. lbmdem_contact_stats and a download with too little room or with room 0 count only and
 * leave the buffer as the last emit wrote it. */
#define LBMDEM_WALL_B (-1)   /* bottom, force_WallB main.c:809 */
#define LBMDEM_WALL_T (-2)   /* top */
#define LBMDEM_WALL_L (-3)   /* left */
#define LBMDEM_WALL_R (-4)   /* right */
typedef struct lbmdem_contact { int i, j; double dn, nx, ny, fn, ft; } lbmdem_contact;   /* 48 bytes */
int lbmdem_contact_stats(lbmdem_handle* h, long* counts6);
int lbmdem_download_contacts(lbmdem_handle* h, lbmdem_contact* out, long cap, long* count);
int lbmdem_write_contacts(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_set_contacts_output(lbmdem_handle* h, int on);            /* 0: off (default) */
int lbmdem_write_contacts_files(const char* dir, int nfile, int n, const double* r, const double* x1, const double* x2,
                                const double* fm, const lbmdem_contact* c, long count, int lx, int ly);   /* host only */
/* Force chains: the contact net above read as a graph, on the device, so that nobody has to download 48 bytes per contact and run
 * a union-find at every DEM event. Which contacts: the records of lbmdem_download_contacts, in that call's order, under that
 * call's validity condition. Nodes are the grains 0 .. n-1; walls are no nodes. Every result is an integer, or a minimum or a
 * maximum, that does not depend on the order of evaluation; a serial restatement over lbmdem_download_contacts and columns 0 and 1
 * of lbmdem_download_grain_table reproduces every number exactly, thr on the bits.
 * 1. Selection. A record is selected iff fn >= thr (never, then, when fn is a NaN). relative == 0: thr = fmin. relative != 0:
 *    thr = fmin * (S / m), where m is the number of grain-grain records with fn > 0 -- converted to double -- and S their sum in this
 *    association: the grain-grain records k = 0, 1, .. in record order are cut into blocks of 1024 consecutive records
 *    (block b holds 1024 b <= k < 1024 (b + 1), the last block may be short); per block a partial, started from +0.0, to which the
 *    block's fn > 0 are added one by one, k ascending (any other record is skipped); S, started from +0.0, to which the partials are
 *    added one by one, b ascending. IEEE double, no contraction. When m == 0: thr = +infinity if fmin > 0, thr = 0 if fmin == 0.
 *    fmin must be finite and >= 0.
 * 2. degree[i]: the selected records that name grain i as i or as j, wall records (j < 0) included. walls[i]: the OR of
 *    1 << (-j - 1) over grain i's selected wall records (LBMDEM_WALL_B 1, _T 2, _L 4, _R 8).
 * 3. label[i]: the smallest grain index in i's connected component over the selected grain-grain records; a grain without a selected
 *    pair is its own label.
 * 4. core[i]: repeat until nothing changes: remove every grain whose remaining degree is < zmin, the remaining degree being the
 *    grain's selected wall records plus its selected pair records whose other end has not been removed. 1 for the survivors, 0
 *    otherwise; the outcome does not depend on the order of removal. zmin lies in 0 .. 6; 0 removes nothing.
 * 5. The cluster table: one lbmdem_cluster per component of size >= 2, ascending label. size: its grains; contacts: the selected pair
 *    records inside it; walls: the OR of its members' walls; core: its members with core == 1; xmin .. ymax: minimum and maximum of
 *    its members' centres, columns 0 and 1 of lbmdem_download_grain_table, under the total order of the bit patterns (-0.0 below
 *    +0.0, a NaN beyond the infinity of its sign). The members of the struct take 56 bytes.
 * 6. counts10, in order: selected pair records; selected wall records; components of size >= 2; size of the largest component (1 if
 *    none has two grains); label of the largest component, the smallest label among equals; grains of degree 0; core grains; selected
 *    pair records with both ends in the core; selected wall records at core grains; the spanning mask -- bit 0: one component has
 *    both LBMDEM_WALL_L and LBMDEM_WALL_R among its walls, bit 1: both LBMDEM_WALL_B and LBMDEM_WALL_T.
 * On the device: one lane per block forms the partials of S and one lane adds them; degree and walls by atomics; the components by
 * min-label hooking (atomicMin on the larger root: a node's parent is never larger than the node, so no cycle can form) and pointer
 * jumping in rounds of kernel launches, the core by rounds that remove and then subtract. Each round raises a device flag when it
 * changed something; the host stops at the first quiet round and gives up, with LBMDEM_EINVAL, after n + 1 rounds. No workgroup
 * waits for another, every device loop has a bound. Scratch comes from the handle's pool with the first call and goes with the
 * handle; everything runs on the handle's stream.
 *   lbmdem_cluster_compute          the analysis of the last table sub-step; counts10 and *thr. Synchronises; changes nothing a
 *                                   later step reads.
 *   lbmdem_download_cluster_grains  label, degree, core, walls, [n] ints each; any pointer may be NULL
 *   lbmdem_cluster_grains_device    the same four as device pointers into the handle's scratch (for a torch view), good until the
 *                                   next compute or lbmdem_destroy; any pointer may be NULL
 *   lbmdem_download_clusters        the table; cap = 0 (out may be NULL) only reports *count; a buffer of fewer than *count entries
 *                                   is refused with *count set
 *   lbmdem_cluster_rounds           rounds2 = the rounds the component loop took (the quiet one included; 0 without a pair record),
 *                                   the rounds of the core loop that removed a grain
 *   These four are refused, with LBMDEM_EINVAL and a sentence that names lbmdem_cluster_compute, when no compute has been made
 *   for the last table sub-step.
 *   lbmdem_write_clusters_files     host only, no handle, no device. Four files in <dir>:
 *                                   clusters%.6i.dat -- "# fmin %le relative %d zmin %d threshold %le\n", "# i label degree core
 *                                   walls\n", then n lines "%d %d %d %d %d\n";
 *                                   cluster_table%.6i.dat -- "%d %d %ld %d %d %le %le %le %le\n" per entry, the members in order;
 *                                   DEM%.6i_clusters.ps -- header and one arc per grain as lbmdem_write_forces prints them, then per
 *                                   selected grain-grain record (fn >= thr) the four lines of DEM%.6i_chains.ps with
 *                                   " <r> <g> <b> setrgbcolor \n" in the place of " 0.0 setgray \n", the colour palette[label[i] % 8]
 *                                   of: "0.894 0.102 0.110", "0.216 0.494 0.722", "0.302 0.686 0.290", "0.596 0.306 0.639",
 *                                   "1.000 0.498 0.000", "0.651 0.337 0.157", "0.969 0.506 0.749", "0.400 0.400 0.400";
 *                                   clusters.data -- one line appended: "%le %le" of t and thr, " %ld" of each of the ten counts,
 *                                   "\n"; when the file is created, first the line "# t threshold selected_pairs selected_walls
 *                                   clusters largest_size largest_label isolated_grains core_grains core_pairs core_walls spanning".
 *                                   It checks fopen; records that name a grain outside [0, n) or an unknown wall, and labels
 *                                   outside [0, n), are refused before anything is written.
 *   lbmdem_write_clusters           the compute, the downloads, then that formatter with r, x1, x2, fm of
 *                                   lbmdem_download_grain_table and t = nbsteps * dt
 *   lbmdem_set_clusters_output      on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_clusters(dir, nFile, fmin, relative,
 *                                   zmin) at every DEM event, behind the contact files. Off by default; a checkpoint does not
 *                                   carry it.
 * LBMDEM_EINVAL: fmin negative or not finite, zmin outside 0 .. 6; a strip of a decomposition or distributed grains (and
 * lbmdem_dist_enable with the setting on); the single-precision library (the host-only formatter exists there too); null buffers; a
 * directory that cannot be written ("cannot open"). What invalidates the contact records invalidates the clusters made of them: a
 * wall that lbmdem_move_walls gives another value, and every lbmdem_verlet_rebuild; compute and readers are refused until the next
 * table sub-step. A compute that is refused for fmin or zmin changes nothing: an earlier result stays readable; one that is refused
 * because the contact records are not valid finds the readers refused already. The kernels read the records in the contact export's
 * buffer, which the compute fills itself; the per-grain planes and the table are the cluster stage's own. No call of the contact
 * export (lbmdem_contact_stats, lbmdem_download_contacts with any room, lbmdem_write_contacts) changes a cluster result, and
 * lbmdem_write_clusters downloads the records of its own compute, right behind it, for DEM%.6i_clusters.ps. */
typedef struct lbmdem_cluster { int label, size; long contacts; int walls, core; double xmin, xmax, ymin, ymax; } lbmdem_cluster;
#define LBMDEM_CLUSTER_COUNTS 10
int lbmdem_cluster_compute(lbmdem_handle* h, double fmin, int relative, int zmin, long* counts10, double* thr);
int lbmdem_download_cluster_grains(lbmdem_handle* h, int* label, int* degree, int* core, int* walls);
int lbmdem_cluster_grains_device(lbmdem_handle* h, const int** label, const int** degree, const int** core, const int** walls);
int lbmdem_download_clusters(lbmdem_handle* h, lbmdem_cluster* out, long cap, long* count);
int lbmdem_cluster_rounds(lbmdem_handle* h, int* rounds2);
int lbmdem_write_clusters(lbmdem_handle* h, const char* dir, int nfile, double fmin, int relative, int zmin);
int lbmdem_set_clusters_output(lbmdem_handle* h, int on, double fmin, int relative, int zmin);   /* 0: off (default) */
int lbmdem_write_clusters_files(const char* dir, int nfile, int n, const double* r, const double* x1, const double* x2,
                                const double* fm, const lbmdem_contact* c, long count, const int* label, const int* degree,
                                const int* core, const int* walls, const lbmdem_cluster* table, long nclusters, double fmin,
                                int relative, int zmin, double thr, const long* counts10, double t, int lx, int ly);   /* host only */
/* Packing structure: what a packing looks like beyond touching partners -- the fixed-radius neighbour list in index order, the pair
 * histogram behind g(r), the bonds of the first shell and the unnormalised bond-order (psi6) and fabric sums -- on the device, so
 * that nobody has to download the centres and run an all-pairs or k-d-tree job at every DEM event. Results are integers wherever
 * possible; where they are floating point, each is a chain of IEEE double operations in the order stated here, which a numpy
 * restatement reproduces on the bits (tests/structure_util.py).
 * Inputs: the current centres x_i, y_i (columns 0 and 1 of lbmdem_download_grain_table, as they are once the handle is settled) and
 * radii r_i (column 9) of the n grains; rcut, finite and > 0, in the unit of the kinematics; nbins in 1 .. 4096; shell, finite and
 * >= 1; max_entries in 0 .. 2^31 - 1. All arithmetic is IEEE double without contraction.
 * 1. Neighbours. dx = x_j - x_i, dy = y_j - y_i, d2 = dx*dx + dy*dy (two products, then one addition), rc2 = rcut*rcut. j is a
 *    neighbour of i iff j != i and d2 <= rc2 -- never, then, with a NaN, and never with an infinite centre; coincident centres are
 *    neighbours. The list is symmetric CSR: offsets[n + 1] ints and nbr[], each grain's neighbours ascending by index.
 * 2. Pair histogram. dr = rcut / nbins; e2[k] = (k*dr)*(k*dr) for k = 0 .. nbins - 1, k converted to double; e2[nbins] = rc2.
 *    hist[k] is the 64-bit count of the unordered neighbour pairs i < j with e2[k] <= d2, and d2 < e2[k + 1] for k < nbins - 1: the
 *    last bin takes everything up to and including rc2. The table alone decides a bin (where neighbouring edges are equal, the last
 *    bin k with e2[k] <= d2); the device guesses with sqrt(d2)/dr and corrects the guess against the table.
 *    lbmdem_structure_edges returns the table, e2[nbins + 1] (host only).
 * 3. Bonds. A neighbour is bonded iff d2 <= b*b with b = shell * (r_i + r_j). bonds[i] is their number.
 * 4. Bond order and fabric. c6[i], s6[i], c2[i], s2[i] start from +0.0; the bonded neighbours with d2 > 0 are added one by one, j
 *    ascending: d = sqrt(d2), nx = dx/d, ny = dy/d; a2 = nx*nx - ny*ny, b2 = 2.*nx*ny; a4 = a2*a2 - b2*b2, b4 = 2.*a2*b2;
 *    a6 = a4*a2 - b4*b2, b6 = b4*a2 + a4*b2; c2 += a2; s2 += b2; c6 += a6; s6 += b6. Unnormalised: |psi6| = sqrt(c6^2 + s6^2) / bonds
 *    and the fabric anisotropy are divisions the caller makes.
 * 5. counts8, in order: list entries (2 x pairs); pairs; bonded pairs (i < j); the largest offsets[i + 1] - offsets[i]; grains
 *    without a neighbour; grains with exactly six bonds; coincident pairs (d2 == 0, i < j); grains with a non-finite centre.
 * Capacity: when the entries exceed max_entries > 0 the compute fails with LBMDEM_EINVAL and a sentence that carries both numbers,
 * and nothing is allocated for the list. max_entries == 0 asks for the counts and the histogram only: the list, bonds and the four
 * sums are not produced and their readers refuse.
 * On the device, all on the handle's stream: a cell grid of the analysis' own over the current centres -- bounds from a min/max over
 * the finite centres, the cell side per axis max(rcut, extent / 1024) and 2^-20 of it more (so that the rounding of a cell index
 * cannot separate two grains at exactly rcut by two cells), the non-finite centres in one cell of their own; the grains ordered by
 * cell with a radix sort; count, scan, emit over the 3 x 3 cells with the candidates staged in LDS 256 at a time (a cell may hold any
 * number of grains); the histogram per workgroup in LDS as 32-bit integers, flushed with 64-bit atomics; a segmented sort for the
 * index order; one lane per grain for the chains of 4. No floating-point atomic, no workgroup waits for another, every loop has a
 * bound. The Verlet list and its grid are not touched. Scratch comes from the handle's pool with the first call.
 *   lbmdem_structure_compute              the compute; counts8. Synchronises; changes nothing a later step reads.
 *   lbmdem_download_structure_grains      nb (= offsets[i + 1] - offsets[i]) and bonds, [n] ints; c6, s6, c2, s2, [n] doubles; any
 *                                         pointer may be NULL
 *   lbmdem_structure_grains_device        the same six as device pointers into the handle's scratch (for a torch view), good until
 *                                         the next compute or lbmdem_destroy; any pointer may be NULL
 *   lbmdem_download_structure_hist        hist[nbins] of the last compute; cap = 0 only reports *nbins; a buffer of fewer bins is
 *                                         refused with *nbins set
 *   lbmdem_download_structure_neighbours  offsets[n + 1] (may be NULL) and nbr[]; cap = 0 leaves nbr alone and reports *count, the
 *                                         entries; a buffer of fewer than *count entries is refused with *count set
 *   These readers are refused, with LBMDEM_EINVAL and a sentence that names lbmdem_structure_compute, until a compute has been
 *   made, and again after anything that moves grains: a sub-step (every kind of step makes some), lbmdem_upload_kinematics; a
 *   checkpoint load gives a new handle, on which no compute has been made. After a compute with max_entries == 0 every reader but
 *   the histogram's refuses.
 *   lbmdem_write_structure_files          host only, no handle, no device. Three files in <dir>:
 *                                         structure%.6i.dat -- "# rcut %le nbins %d shell %le\n", "# i neighbours bonds c6 s6 c2
 *                                         s2\n", then n lines "%d %d %d %le %le %le %le\n" of i, nb, bonds, c6, s6, c2, s2;
 *                                         gr%.6i.dat -- "# rcut %le nbins %d n %d W %le H %le\n", a second "#" line that states g,
 *                                         then per bin "%d %le %le %ld %le\n" of k, sqrt(e2[k]), sqrt(e2[k + 1]), hist[k] and
 *                                         g = hist[k] / ideal, ideal = ((npairs_all * pi) * (e2[k + 1] - e2[k])) / (W * H) in
 *                                         this association, npairs_all = ((double)n * (double)(n - 1)) / 2., pi =
 *                                         3.141592653589793; g = 0 where ideal is no positive number. No edge correction;
 *                                         structure.data -- one line appended: "%le" of t, " %ld" of each of the eight counts,
 *                                         " %le %le\n" of psi6 and fabric. psi6: the sum, from +0.0 and by index, of
 *                                         sqrt(c6*c6 + s6*s6) / bonds over the grains with bonds, divided by their number (0
 *                                         without one); fabric: sqrt(C2*C2 + S2*S2) / B with C2, S2 the sums of c2, s2 from +0.0
 *                                         by index and B the sum of bonds (0 when B is 0). When the file is created, first the line
 *                                         "# t entries pairs bonded_pairs max_neighbours lone_grains six_bonds coincident_pairs
 *                                         nonfinite_grains psi6 fabric". It checks fopen; nb outside [0, n), bonds outside
 *                                         [0, nb] and a negative bin are refused before anything is written.
 *   lbmdem_write_structure                the compute with max_entries = 2^31 - 1, the downloads, then that formatter with
 *                                         t = nbsteps * dt, W = Mdx - Mgx and H = Mhy - Mby, where the walls stand
 *   lbmdem_set_structure_output           on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_structure(dir, nFile, rcut,
 *                                         nbins, shell) at every DEM event, behind the cluster files. Off by default; a checkpoint
 *                                         does not carry it.
 * Single-domain fp64 handles; vibrating, probing, lid, tracer, scalar and mean handles included. LBMDEM_EINVAL: a parameter outside
 * its range; a strip of a decomposition or distributed grains (and lbmdem_dist_enable with the setting on); the single-precision
 * library (the two host-only functions exist there too); null buffers; a directory that cannot be written ("cannot open"). A later
 * compute replaces the result whole -- list, histogram, sums, rcut, nbins and whether there is a list --; one that is refused for a
 * parameter changes nothing, one whose list exceeds max_entries leaves no result. lbmdem_write_structure and lbmdem_write_voronoi
 * make computes of their own: after lbmdem_write_voronoi(rcut) the readers describe lbmdem_structure_compute(rcut, 1, 1.0), and
 * so they do after a DEM event of lbmdem_run_scene with both outputs on, where the structure files, written first, are those of
 * lbmdem_set_structure_output's parameters and the Voronoi files those of lbmdem_set_voronoi_output's rcut. */
#define LBMDEM_STRUCTURE_COUNTS 8
int lbmdem_structure_edges(double rcut, int nbins, double* e2);   /* host only */
int lbmdem_structure_compute(lbmdem_handle* h, double rcut, int nbins, double shell, long max_entries, long* counts8);
int lbmdem_download_structure_grains(lbmdem_handle* h, int* nb, int* bonds, double* c6, double* s6, double* c2, double* s2);
int lbmdem_structure_grains_device(lbmdem_handle* h, const int** nb, const int** bonds, const double** c6, const double** s6,
                                   const double** c2, const double** s2);
int lbmdem_download_structure_hist(lbmdem_handle* h, long* hist, int cap, int* nbins);
int lbmdem_download_structure_neighbours(lbmdem_handle* h, int* offsets, int* nbr, long cap, long* count);
int lbmdem_write_structure(lbmdem_handle* h, const char* dir, int nfile, double rcut, int nbins, double shell);
int lbmdem_set_structure_output(lbmdem_handle* h, int on, double rcut, int nbins, double shell);   /* 0: off (default) */
int lbmdem_write_structure_files(const char* dir, int nfile, int n, const int* nb, const int* bonds, const double* c6,
                                 const double* s6, const double* c2, const double* s2, double rcut, int nbins, double shell,
                                 const long* hist, const long* counts8, double t, double W, double H);   /* host only */
/* Voronoi cells: how much space a grain has -- the radical (power, Laguerre) tessellation of the discs inside the four walls, on the
 * device and on top of the neighbour list the structure analysis leaves there: per grain the cell's area, perimeter and local solid
 * fraction, its topological neighbour count and the walls it touches, and the cells' faces as CSR -- the Delaunay graph with the
 * length of every face. Every floating-point result is a chain of IEEE double operations in the order stated here, which a Python
 * restatement reproduces on the bits (tests/voronoi_util.py).
 * Inputs: the centres x_i, y_i and radii r_i as the structure analysis reads them; the four walls where they stand now, Mgx, Mdx,
 * Mby, Mhy of lbmdem_get_config (on a vibrating handle the moved walls); offsets, nbr and rcut of the most recent
 * lbmdem_structure_compute, which must still be valid and must have made a list (the handle keeps rcut*rcut, the last edge of
 * that compute's table; squaring is one-to-one on doubles with a normal square, so rcut is the one double whose square rounds to
 * it, and a compute whose rcut*rcut is no normal number is refused); rmax, the largest r_i (a max is exact in any order). All
 * arithmetic is IEEE double without contraction, the operations in the order written here.
 * 1. The cell of grain i is a convex polygon of at most LBMDEM_VOR_MAXV = 32 vertices; vertex k carries (vx, vy) and src, the source
 *    of the edge that leaves it towards vertex k + 1 (cyclically): a grain's index, or -1 .. -4 for the bottom, right, top and left
 *    wall. It starts as the box, counter-clockwise: (Mgx, Mby, -1) (Mdx, Mby, -2) (Mdx, Mhy, -3) (Mgx, Mhy, -4). A grain with a
 *    non-finite centre starts with no vertices.
 * 2. The polygon is clipped by each neighbour j of the list, in list order (ascending index), while it has vertices:
 *    dx = x_j - x_i, dy = y_j - y_i, d2 = dx*dx + dy*dy; j is skipped unless d2 > 0. h = 0.5*((d2 + r_i*r_i) - r_j*r_j). For every
 *    vertex s = ((vx - x_i)*dx + (vy - y_i)*dy) - h; the vertex is inside iff s <= 0. The edges a -> b are walked in order: if a is
 *    inside, a is emitted with its own src; if exactly one of a, b is inside, t = sa/(sa - sb) and the vertex
 *    (a.vx + t*(b.vx - a.vx), a.vy + t*(b.vy - a.vy)) is emitted with src = j when a is inside, else a.src. A line that cuts nothing
 *    (every vertex inside) leaves the polygon as it was -- the device may therefore pass over a j of which a bound shows that
 *    every s is negative. A clip that would leave more than 32 vertices overflows the cell: no vertices, flag OVERFLOW.
 * 3. Measures, one walk over the final polygon, sums from +0.0: with ax = a.vx - x_i, ay = a.vy - y_i and bx, by alike,
 *    A2 += ax*by - bx*ay and area = 0.5*A2; with ex = b.vx - a.vx, ey = b.vy - a.vy, len = sqrt(ex*ex + ey*ey) and
 *    perimeter += len; R2 = max(ax*ax + ay*ay), from 0. An edge is a face iff its two endpoints differ in either coordinate,
 *    compared on values (lattices make edges of no length, and those must not count). faces counts the faces with src >= 0, walls
 *    is the OR of 1 << (-src - 1) over the faces with src < 0, nverts the vertices. phi = ((pi*r_i)*r_i)/area where area > 0, else
 *    0, pi = 3.141592653589793. A cell without vertices has zeros in every measure.
 * 4. flags: LBMDEM_VOR_EMPTY -- no vertices left and not overflowed (a non-finite centre too); LBMDEM_VOR_OVERFLOW;
 *    LBMDEM_VOR_NONFINITE -- the centre; LBMDEM_VOR_COMPLETE -- with bound = 0.5*(rcut + (r_i*r_i - rmax*rmax)/rcut), set iff
 *    nverts > 0 && bound > 0 && R2 <= bound*bound. Then no grain beyond the cutoff could cut the cell: a point p of the cell has
 *    |p - x_i| <= bound =: b, a grain j outside the list has |x_j - x_i| > rcut, hence |p - x_j| > rcut - b, and j's power
 *    (rcut - b)^2 - rmax^2 = b^2 - r_i^2 + (rcut^2 - 2 rcut b - rmax^2 + r_i^2) = b^2 - r_i^2 is no smaller than i's own.
 * 5. Faces as CSR: foff[n + 1] is the scan of the number of faces of either kind; per face, in polygon order, fsrc (the neighbour,
 *    or -1 .. -4) and flen (len above). j is a Delaunay neighbour of i where j is in i's segment of fsrc.
 * 6. counts8, in order: cells with area > 0; complete cells; empty cells; overflowed cells; grains with a non-finite centre; grain
 *    faces, counted from both sides; wall faces; the largest faces.
 * On the device, on the handle's stream: one lane per grain clips its own cell serially, the polygon (twice: the one it clips, the
 * one it makes) in an LDS slice of its own; the faces go to rows, a scan makes foff, an emit fills the CSR; the census is integer
 * atomics. No floating-point atomic, no workgroup waits for another, every loop has a bound. The kernels read the structure
 * analysis' list and the kinematics and write to scratch of their own, taken from the handle's pool with the first call.
 *   lbmdem_voronoi_compute          the compute; counts8. Synchronises; changes nothing a later step reads. Refused with a sentence
 *                                   that names lbmdem_structure_compute when no such compute describes the grains where they are now,
 *                                   or when the last one had max_entries == 0.
 *   lbmdem_download_voronoi_grains  area, perimeter, phi, R2, [n] doubles; faces, walls, nverts, flags, [n] ints; any pointer may
 *                                   be NULL
 *   lbmdem_voronoi_grains_device    the same eight as device pointers into the handle's scratch (for a torch view), good until the
 *                                   next compute or lbmdem_destroy; any pointer may be NULL
 *   lbmdem_download_voronoi_faces   foff[n + 1] (may be NULL), fsrc[] and flen[] (either may be NULL); cap = 0 leaves both alone and
 *                                   reports *count, the faces; buffers of fewer than *count faces are refused with *count set
 *   These readers are refused, with LBMDEM_EINVAL and a sentence that names lbmdem_voronoi_compute, until a compute has been made,
 *   and again after anything that moves grains, exactly as the structure readers are.
 *   lbmdem_write_voronoi_files      host only, no handle, no device. Two files in <dir>: voronoi%.6i.dat -- "# rcut %le\n",
 *                                   "# i area perimeter phi faces walls nverts flags\n", then n lines "%d %le %le %le %d %d %d %d\n";
 *                                   voronoi.data -- one line appended: "%le" of t, " %ld" of each of the eight counts,
 *                                   " %le %le %le %le\n" of the sum of area from +0.0 by index, W*H, the mean phi over the complete
 *                                   cells with area > 0 (their phi added from +0.0 by index, divided by their number; 0 without
 *                                   one) and the mean faces over the same cells (faces converted to double, added and divided
 *                                   alike). When the file is created, first the line "# t cells complete empty overflowed
 *                                   nonfinite_grains grain_faces wall_faces max_faces sum_area box_area mean_phi mean_faces". It
 *                                   checks fopen; nverts outside [0, 32] and faces outside [0, nverts] are refused before anything
 *                                   is written.
 *   lbmdem_write_voronoi            lbmdem_structure_compute(rcut, 1, 1.0, 2^31 - 1), the Voronoi compute, the downloads, then that
 *                                   formatter with t = nbsteps * dt, W = Mdx - Mgx and H = Mhy - Mby, where the walls stand
 *   lbmdem_set_voronoi_output       on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_voronoi(dir, nFile, rcut) at every
 *                                   DEM event, behind the structure files. Off by default; a checkpoint does not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL: rcut not finite and > 0; a strip of a decomposition or distributed grains (and
 * lbmdem_dist_enable with the setting on); the single-precision library (the host-only formatter exists there too); null buffers;
 * a directory that cannot be written ("cannot open"). The cells are clipped with Mgx, Mdx, Mby, Mhy as the compute finds them: a
 * wall that changes value afterwards without a sub-step (lbmdem_move_walls, lbmdem_verlet_rebuild) invalidates them, and the
 * readers are refused as after a move of the grains until the next lbmdem_voronoi_compute (the neighbour list stays good). The cells
 * are the Voronoi stage's own: a later lbmdem_structure_compute (another rcut or nbins, counts only, refused) leaves the readers
 * answering with the cells of the list and the rcut they were made with, until a grain or a wall moves. A refused
 * lbmdem_voronoi_compute (no valid list, a counts-only list) discards an earlier result: the readers are refused until the next
 * compute that succeeds. lbmdem_write_voronoi writes its own argument as "# rcut"; its lbmdem_structure_compute(rcut, 1, 1.0,
 * 2^31 - 1) replaces the structure result. Afterwards the structure readers describe that compute, not an earlier one. */
#define LBMDEM_VORONOI_COUNTS 8
#define LBMDEM_VOR_MAXV 32
#define LBMDEM_VOR_COMPLETE 1
#define LBMDEM_VOR_EMPTY 2
#define LBMDEM_VOR_OVERFLOW 4
#define LBMDEM_VOR_NONFINITE 8
int lbmdem_voronoi_compute(lbmdem_handle* h, long* counts8);
int lbmdem_download_voronoi_grains(lbmdem_handle* h, double* area, double* perimeter, double* phi, double* R2, int* faces, int* walls,
                                   int* nverts, int* flags);
int lbmdem_voronoi_grains_device(lbmdem_handle* h, const double** area, const double** perimeter, const double** phi,
                                 const double** R2, const int** faces, const int** walls, const int** nverts, const int** flags);
int lbmdem_download_voronoi_faces(lbmdem_handle* h, int* foff, int* fsrc, double* flen, long cap, long* count);
int lbmdem_write_voronoi(lbmdem_handle* h, const char* dir, int nfile, double rcut);
int lbmdem_set_voronoi_output(lbmdem_handle* h, int on, double rcut);   /* 0: off (default) */
int lbmdem_write_voronoi_files(const char* dir, int nfile, int n, const double* area, const double* perimeter, const double* phi,
                               const int* faces, const int* walls, const int* nverts, const int* flags, double rcut,
                               const long* counts8, double t, double W, double H);   /* host only */
/* Strain fields: what has happened to the packing since a reference state -- per grain the displacement, the deformation gradient F
 * of its neighbourhood (a least-squares fit over the neighbours it had at the reference state), Falk and Langer's D2min (the part of
 * the neighbours' motion that F does not explain: the marker of plastic rearrangements) and the neighbours it has lost. Every
 * floating-point result is a chain of IEEE double operations in the order stated here, which a numpy restatement reproduces on the
 * bits (tests/strain_util.py).
 * The mark (the reference configuration). lbmdem_strain_mark copies into scratch of the stage's own: the current x1, x2, x3 of the
 * n grains (columns 0, 1, 2 of lbmdem_download_grain_table); offsets[n + 1], nbr[] (each grain's neighbours ascending) and
 * rc2 = rcut*rcut of the most recent lbmdem_structure_compute, which must still be valid for the grains where they are and must
 * have made a list; nbsteps. It makes no structure compute of its own. It is a copy: nothing the structure or the Voronoi analysis
 * do later changes it. A mark lives until the next successful mark, lbmdem_strain_clear or lbmdem_destroy; steps,
 * lbmdem_upload_kinematics and wall moves do not end it; a checkpoint does not carry it and a loaded handle has none. A new mark
 * and a clear discard the compute's result; a refused mark leaves the earlier mark and its result as they were.
 * The compute. X0, Y0, T0: the marked x1, x2, x3; x, y, th: the current ones. All arithmetic is IEEE double without contraction,
 * the operations in the order written here. Per grain i:
 * 1. LBMDEM_STRAIN_NONFINITE iff any of x_i, y_i, X0_i, Y0_i is not finite. Then flags = 1, used = lost = 0, every double output
 *    of i is +0.0 and 2 to 4 are skipped. Otherwise ux = x_i - X0_i, uy = y_i - Y0_i, drot = th_i - T0_i.
 * 2. Pass 1 over i's marked neighbours j in list order, the seven sums from +0.0: d0x = X0_j - X0_i, d0y = Y0_j - Y0_i,
 *    dx = x_j - x_i, dy = y_j - y_i. j is skipped unless dx and dy are finite. Otherwise used += 1, and lost += 1 where
 *    dx*dx + dy*dy > rc2; Xxx += dx*d0x; Xxy += dx*d0y; Xyx += dy*d0x; Xyy += dy*d0y; Yxx += d0x*d0x; Yxy += d0x*d0y;
 *    Yyy += d0y*d0y.
 * 3. Fit. det = Yxx*Yyy - Yxy*Yxy. LBMDEM_STRAIN_FEW iff used < 2; LBMDEM_STRAIN_DEGENERATE iff not FEW and not
 *    det > 0x1p-40*(Yxx*Yyy) (collinear neighbours; a NaN too). With either flag Fxx, Fxy, Fyx, Fyy and d2min are +0.0 and 4 is
 *    skipped. Otherwise Ixx = Yyy/det; Ixy = (-Yxy)/det; Iyy = Yxx/det; Fxx = Xxx*Ixx + Xxy*Ixy; Fxy = Xxx*Ixy + Xxy*Iyy;
 *    Fyx = Xyx*Ixx + Xyy*Ixy; Fyy = Xyx*Ixy + Xyy*Iyy. A grain without a flag is "fitted".
 * 4. Pass 2 over the same neighbours with the same skip rule, d2min from +0.0: rx = dx - (Fxx*d0x + Fxy*d0y);
 *    ry = dy - (Fyx*d0x + Fyy*d0y); d2min += rx*rx + ry*ry. Unnormalised: dividing by used is the caller's.
 * 5. counts8, in order: fitted grains (flags == 0); FEW; DEGENERATE; NONFINITE; marked list entries; entries used (the sum of used);
 *    entries lost (the sum of lost); the index of the fitted grain with the largest d2min, the smallest index among equals, -1
 *    without a fitted grain. "Largest" is by the key of d2min: its bit pattern as an unsigned 64-bit integer where d2min >= +0.0
 *    -- the order of the values --, and 0 otherwise (a NaN counts as +0.0).
 * On the device, on the handle's stream: a packing pass writes one 32-byte record {X0, Y0, x, y} per grain, so that a neighbour
 * costs two 16-byte loads; one lane per grain walks its segment of the marked list twice, serially; the census is integer
 * atomics, the argmax an integer atomicMax over the keys and an atomicMin over the indices that carry the maximum. No
 * floating-point atomic, no workgroup waits for another, every loop is bounded by the segment length. Scratch comes from the
 * handle's pool with the first mark.
 *   lbmdem_strain_mark                the mark; *entries (may be NULL): the list entries copied. Synchronises; changes nothing a later
 *                                     step reads. Refused with a sentence that names lbmdem_structure_compute when no such compute
 *                                     describes the grains where they are now, or when the last one had max_entries == 0.
 *   lbmdem_strain_clear               no mark and no result any more (the scratch stays with the handle)
 *   lbmdem_strain_compute             the compute; counts8. Synchronises; changes nothing a later step reads. Without a mark it is
 *                                     refused with a sentence that names lbmdem_strain_mark, and an earlier result is discarded.
 *   lbmdem_download_strain_grains     ux, uy, drot, Fxx, Fxy, Fyx, Fyy, d2min, [n] doubles; used, lost, flags, [n] ints; any pointer
 *                                     may be NULL
 *   lbmdem_strain_grains_device       the same eleven as device pointers into the handle's scratch (for a torch view), good until
 *                                     the next compute or lbmdem_destroy; any pointer may be NULL
 *   These two readers are refused, with LBMDEM_EINVAL and a sentence that names lbmdem_strain_compute, until a compute has been
 *   made, and again after anything that moves grains (a sub-step, lbmdem_upload_kinematics), after a new mark and after a clear.
 *   A wall that moves without a sub-step does not invalidate the result: walls do not enter.
 *   lbmdem_download_strain_reference  the mark: x0, y0, th0, [n] doubles, offsets[n + 1] (any of the four may be NULL) and nbr[];
 *                                     *rc2 and *nbsteps (either may be NULL); cap = 0 leaves nbr alone and reports *count, the
 *                                     entries; a buffer of fewer than *count entries is refused with *count set. Good whenever a
 *                                     mark exists, compute or not; refused with a sentence that names lbmdem_strain_mark otherwise.
 *   lbmdem_write_strain_files         host only, no handle, no device. Two files in <dir>: strain%.6i.dat -- "# rc2 %le t_mark
 *                                     %le\n", "# i ux uy drot exx eyy exy omega vol dev d2min used lost flags\n", then n lines
 *                                     "%d %le %le %le %le %le %le %le %le %le %le %d %d %d\n". For a fitted grain exx = Fxx - 1.,
 *                                     eyy = Fyy - 1., exy = 0.5*(Fxy + Fyx), omega = 0.5*(Fyx - Fxy), vol = exx + eyy,
 *                                     h = 0.5*(exx - eyy), dev = sqrt(h*h + exy*exy); otherwise all six are 0.
 *                                     strain.data -- one line appended: "%le" of t, " %ld" of each of the eight counts,
 *                                     " %le %le %le\n" of the mean squared displacement (ux*ux + uy*uy added from +0.0 by index
 *                                     over the grains without NONFINITE, divided by their number; 0 without one), the mean of
 *                                     d2min/used over the fitted grains (added and divided alike) and the largest d2min of a
 *                                     fitted grain (from 0., by index, replaced where d2min is greater). When the file is
 *                                     created, first the line "# t fitted few degenerate nonfinite_grains entries used lost
 *                                     worst_grain msd mean_d2min max_d2min". It checks fopen; used outside [0, n), lost outside
 *                                     [0, used] and flags outside 0 .. 7 are refused before anything is written.
 *   lbmdem_write_strain               without a mark, first lbmdem_structure_compute(rcut, 1, 1.0, 2^31 - 1) and the mark (the
 *                                     files then describe the mark against itself); the compute, the downloads, then that
 *                                     formatter with the mark's rc2, t = nbsteps * dt and t_mark = the mark's nbsteps * dt; with
 *                                     incremental != 0, afterwards the same structure compute and a new mark, so that the next
 *                                     call describes the motion since this one
 *   lbmdem_set_strain_output          on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_strain(dir, nFile, rcut,
 *                                     incremental) at every DEM event, behind the Voronoi files. Off by default; nothing is
 *                                     allocated or launched while it is off; a checkpoint does not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL: rcut not finite and > 0; a strip of a decomposition or distributed grains (and
 * lbmdem_dist_enable with the setting on); the single-precision library (the host-only formatter exists there too); null buffers;
 * a directory that cannot be written ("cannot open"). lbmdem_write_strain's lbmdem_structure_compute(rcut, 1, 1.0, 2^31 - 1) --
 * made when there is no mark, and again with incremental != 0 -- replaces the structure result. Afterwards the structure readers
 * describe that compute, not an earlier one; with a mark and incremental == 0 the structure result is left alone. */
#define LBMDEM_STRAIN_COUNTS 8
#define LBMDEM_STRAIN_NONFINITE 1
#define LBMDEM_STRAIN_FEW 2
#define LBMDEM_STRAIN_DEGENERATE 4
int lbmdem_strain_mark(lbmdem_handle* h, long* entries);
int lbmdem_strain_clear(lbmdem_handle* h);
int lbmdem_strain_compute(lbmdem_handle* h, long* counts8);
int lbmdem_download_strain_grains(lbmdem_handle* h, double* ux, double* uy, double* drot, double* Fxx, double* Fxy, double* Fyx,
                                  double* Fyy, double* d2min, int* used, int* lost, int* flags);
int lbmdem_strain_grains_device(lbmdem_handle* h, const double** ux, const double** uy, const double** drot, const double** Fxx,
                                const double** Fxy, const double** Fyx, const double** Fyy, const double** d2min, const int** used,
                                const int** lost, const int** flags);
int lbmdem_download_strain_reference(lbmdem_handle* h, double* x0, double* y0, double* th0, int* offsets, int* nbr, long cap,
                                     long* count, double* rc2, long* nbsteps);
int lbmdem_write_strain(lbmdem_handle* h, const char* dir, int nfile, double rcut, int incremental);
int lbmdem_set_strain_output(lbmdem_handle* h, int on, double rcut, int incremental);   /* 0: off (default) */
int lbmdem_write_strain_files(const char* dir, int nfile, int n, const double* ux, const double* uy, const double* drot,
                              const double* Fxx, const double* Fxy, const double* Fyx, const double* Fyy, const double* d2min,
                              const int* used, const int* lost, const int* flags, double rc2, const long* counts8, double t,
                              double t_mark);   /* host only */
/* Pore space: is the fluid connected? In two dimensions touching discs close the gaps between them, and whether a reductionR, a
 * lattice resolution and a packing leave one percolating pore space or a set of sealed pockets decides whether the pore pressures
 * mean anything. The fluid phase of the obstacle map is labelled into connected components on the device; per component its size,
 * extent, the walls it touches, its wetted links and its fluid mass; per grain the pores it borders -- a grain that borders two
 * different pores plugs a throat. Every result is an integer and the labels are canonical, so nothing depends on the algorithm; a
 * numpy restatement reproduces everything exactly (tests/pore_util.py).
 * Inputs, as of the call: the map M, lbmdem_download_obst's [lx][ly] or a caller's map of that shape, and f, lbmdem_download_f's.
 * Node (x, y) has the index k = x*ly + y. lx*ly (and lx times the device's row pitch, ly rounded up to 16) must be below 2^31. A
 * node is fluid iff M == -1, a grain node iff 0 <= M < nbgrains, a wall node iff M == nbgrains; a caller's map with any other value
 * is refused before any result exists, the sentence names the first offending index.
 * 1. Components. conn is 4 or 8. Two fluid nodes are joined when they differ by one of the directions q = 1..8 of the D2Q9 set
 *    (conn == 4: the axis directions q = 2, 4, 6, 8 only). With conn == 8 a diagonal step joins them whatever the other two nodes
 *    of the square are: exactly what streaming lets a population cross. label[x][y] is the smallest index k of the node's
 *    component, -1 where the node is not fluid.
 * 2. Table: one lbmdem_pore per component, ascending by label. nodes; xmin, xmax, ymin, ymax over its nodes; grain_links and
 *    wall_links: the pairs (fluid node of the component, q in 1..8 -- always all eight) whose neighbour is a grain node, or is a wall
 *    node or lies outside the lattice; walls: for every such wall or outside neighbour (nx, ny) bit 0 (B) if ny <= 0, bit 1 (T)
 *    if ny >= ly - 1, bit 2 (L) if nx <= 0, bit 3 (R) if nx >= lx - 1; mass_q32: per fluid node rho = 0. + f0 + .. + f8
 *    (lbmdem_download_macro's value); where rho is finite and |rho| < 2^20 the node adds (long)rint(rho * 4294967296.), ties to
 *    even, in 64-bit two's-complement arithmetic that wraps; otherwise it adds 0 and is counted under 4. Fixed point: the sum does
 *    not depend on the order and needs integer atomics only.
 * 3. Per grain, [n] ints each: wet, the pairs (node of grain i, q in 1..8) whose neighbour lies inside the lattice and is fluid;
 *    pore_min and pore_max, the smallest and the largest label among those neighbours, both -1 when there is none. With a caller's
 *    map grain i's nodes are that map's.
 * 4. counts10, in order: fluid nodes; components; nodes of the largest component (0 if none); its label (the smallest among equals,
 *    -1 if none); fluid nodes outside the largest component (the trapped ones); components of exactly one node; spanning mask: bit
 *    0 when a component carries both L and R, bit 1 when one carries both B and T; grains with pore_min != pore_max; grains with
 *    wet == 0; fluid nodes whose rho was not accumulated.
 * On the device, on the handle's stream, in the device layout (node = x*sy + y, the same order as k): k_po_local labels a tile of
 * 16 x 64 nodes in LDS by a union-find and stores per fluid node the tile's smallest node of its component; k_po_seam joins across
 * the tiles' borders, one lane per border node, by atomicMin on the larger root; k_po_flatten sets every node to its root and
 * counts the roots, a scan and k_po_emit rank them in ascending order; k_po_table accumulates table and grain outputs with integer
 * atomics behind a reduction over the lanes of a wavefront that share a label and an LDS slot per workgroup. A parent is never
 * larger than its node: a find walks strictly downward, no cycle can form, a union retries only when another lane has lowered
 * the same root. Single launches, no workgroup waits for another, no floating-point atomic. Scratch comes from the handle's pool
 * with the first call and goes with the handle.
 *   lbmdem_pore_compute          the compute; map NULL: the handle's; counts10. Synchronises; changes nothing a later step reads.
 *   lbmdem_download_pore_labels  label[lx][ly]
 *   lbmdem_pore_labels_device    the label plane where it lies on the device, node (x, y) at x * *sy + y (for a torch view), good
 *                                until the next compute or lbmdem_destroy
 *   lbmdem_download_pores        the table; cap = 0 leaves `out` alone and reports *count; a buffer of fewer than *count entries is
 *                                refused with *count set and nothing written
 *   lbmdem_download_pore_grains  wet, pore_min, pore_max, [n] ints; any pointer may be NULL
 *   lbmdem_pore_grains_device    the same three as device pointers; any pointer may be NULL
 *   These readers are refused, with LBMDEM_EINVAL and a sentence that names lbmdem_pore_compute, until a compute has been made, and
 *   again after anything that changes the map or f: any kind of step or sub-step, lbmdem_upload_f, lbmdem_upload_kinematics.
 *   lbmdem_write_pore_files      host only, no handle, no device. In <dir>: pore_table%.6i.dat -- "# conn %d lx %d ly %d\n",
 *                                "# label nodes xmin xmax ymin ymax grain_links wall_links walls mass_q32\n", then per entry
 *                                "%d %ld %d %d %d %d %ld %ld %d %ld\n"; pore_grains%.6i.dat -- "# i wet pore_min pore_max\n", then n
 *                                lines "%d %d %d %d\n"; pores.data -- one line appended, "%le" of t and " %ld" of each of the ten
 *                                counts; when the file is created, first the line "# t fluid_nodes components largest_nodes
 *                                largest_label trapped_nodes single_nodes spanning throat_grains dry_grains unaccumulated";
 *                                pores%.6i.vtk, only when plane != 0 -- the label plane as legacy STRUCTURED_POINTS on the frames'
 *                                mesh, lbmdem_write_scalar_files' header with the title "lbmdem pore labels" and "SCALARS pore int
 *                                1", then the labels as big-endian 32-bit integers, x fastest. It checks fopen ("cannot open");
 *                                labels outside [-1, lx*ly) and table entries not ascending by label are refused before anything
 *                                is written. label may be NULL when plane == 0, table when ntable == 0.
 *   lbmdem_write_pores           the compute on the handle's map, the downloads, then that formatter with t = nbsteps * dt
 *   lbmdem_set_pores_output      on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_pores(dir, nFile, conn, plane) at
 *                                every DEM event, behind the Voronoi files. Off by default; a checkpoint does not carry it.
 * Single-domain fp64 handles, vibrating, probing, lid, tracer, scalar and mean handles included. LBMDEM_EINVAL: conn other than 4 or
 * 8; null arguments; a lattice of 2^31 nodes or more; a strip of a decomposition or distributed grains (and lbmdem_dist_enable with
 * the setting on); the single-precision library (the host-only formatter exists there too); a directory that cannot be written. */
typedef struct lbmdem_pore {
  int label, walls;
  long nodes, grain_links, wall_links, mass_q32;
  int xmin, xmax, ymin, ymax;
} lbmdem_pore;
#define LBMDEM_PORE_COUNTS 10
int lbmdem_pore_compute(lbmdem_handle* h, int conn, const int* map /* NULL: the handle's */, long* counts10);
int lbmdem_download_pore_labels(lbmdem_handle* h, int* label);   /* [lx][ly], host layout */
int lbmdem_pore_labels_device(lbmdem_handle* h, const int** label, int* sy);   /* device layout, pitch sy */
int lbmdem_download_pores(lbmdem_handle* h, lbmdem_pore* out, long cap, long* count);
int lbmdem_download_pore_grains(lbmdem_handle* h, int* wet, int* pore_min, int* pore_max);   /* any may be NULL */
int lbmdem_pore_grains_device(lbmdem_handle* h, const int** wet, const int** pore_min, const int** pore_max);
int lbmdem_write_pores(lbmdem_handle* h, const char* dir, int nfile, int conn, int plane);
int lbmdem_set_pores_output(lbmdem_handle* h, int on, int conn, int plane);   /* 0: off (default) */
int lbmdem_write_pore_files(const char* dir, int nfile, int conn, int lx, int ly, int plane, const int* label,
                            const lbmdem_pore* table, long ntable, int n, const int* wet, const int* pore_min,
                            const int* pore_max, const long* counts10, double t);   /* host only */
/* Pore clearance: how WIDE is the pore space? The pore-size distribution, the narrowest gap between every two neighbouring grains
 * -- the throat that sets the permeability and closes first -- and the grain every fluid node belongs to, all from one exact
 * integer object: the squared Euclidean distance from each fluid node to the nearest position that is not fluid, with that
 * position's owner. Every result is an integer and every tie has a rule, so nothing depends on the algorithm; a numpy restatement
 * reproduces everything exactly (tests/clearance_util.py) and its distances are scipy.ndimage.distance_transform_edt's.
 * Input, as of the call: the map M, lbmdem_download_obst's [lx][ly] or a caller's map of that shape: -1 fluid, 0 .. n-1 a grain,
 * n = nbgrains the wall; a caller's map with any other value is refused before any result exists, the sentence names the first
 * offending index (lbmdem_pore_compute's sentence). Node (x, y) has the index k = x*ly + y. Every position outside the lattice
 * counts as a wall node, owner n. lx and ly are at most 32768, so that d2 < 2^31.
 * 1. d2[x][y], int: for a fluid node the minimum over all positions (x', y') that are not fluid, those outside the lattice
 *    included, of (x-x')^2 + (y-y')^2; 0 off the fluid.
 * 2. owner[x][y], int: for a fluid node the smallest map value among the non-fluid positions at distance exactly d2 -- a grain
 *    before the wall, the smaller grain index among grains; off the fluid M itself.
 * 3. hist[k], long, k = 0 .. kmax: the fluid nodes with isqrt(d2) == k, isqrt the integer square root rounded down,
 *    kmax = isqrt(the largest d2): the pore-size distribution. (hist[0] is 0.)
 * 4. Per owner 0 .. n, entry n the wall: owned, long, the fluid nodes that have this owner; d2max, int, the largest d2 among them,
 *    -1 without one.
 * 5. Ridge edges: the pairs of fluid nodes p < q, q = p + 1 in the same row x or q = p + ly, with owner[p] != owner[q]. An edge's
 *    pair is (lo, hi) = (min, max) of the two owners, its clearance c = max(d2[p], d2[q]). The throat table: one lbmdem_throat per
 *    distinct pair, ascending by (lo, hi): edges, the number of the pair's edges (the length of the ridge between the two); c_min,
 *    the smallest clearance among them; node, the smallest p among the edges with c == c_min. Two discs whose nearest nodes are an
 *    even g apart have c_min = (g/2)^2.
 * 6. counts10, in order: fluid_nodes; d2_max, the largest d2 of the lattice (0 without fluid); d2_max_node, the smallest index k
 *    with d2 == d2_max; sum_d2, the sum over all nodes; ridge_edges; throats, the table's entries; grain_throats, those with
 *    hi < n; narrowest_c, the smallest c_min of those, -1 without one; ownerless_grains, the grains 0 .. n-1 with owned == 0;
 *    kmax.
 * On the device, on the handle's stream, in the device layout (node = x*sy + y): one packed key per node, d2 << 32 | owner, whose
 * minimum is the rule of 1 and 2. k_ce_row, a wavefront per row x, finds the nearest non-fluid position of the row below and
 * above every y by running maxima and minima over the lanes (the positions -1 and ly seed them) and stores g^2 << 32 | owner;
 * k_ce_col, lanes along y, lets every node walk x' = x -+ 1, x -+ 2, .. over the rows' keys, rows outside the lattice counting as
 * dx^2 << 32 | n, until dx^2 exceeds the best distance -- exact, because the nearest non-fluid position within row x' is that
 * row's nearest along y -- writes d2 and owner and accumulates the histogram and the owners' table (lanes of a wavefront that
 * share a bin or an owner first, then LDS, then 64-bit integer atomics); k_ce_count, a scan and k_ce_emit list the ridge edges
 * as (pair, c, p) records, two stable radix sorts order them by pair, c and p, a run-length encode finds the pairs and
 * k_ce_throats reads each run's first record; k_ce_census makes the counts. Single launches, integer atomics only, no floating
 * point. Scratch comes from the handle's pool with the first call and goes with the handle; the ridge records are allocated for
 * the edges there are.
 *   lbmdem_clearance_compute        the compute; map NULL: the handle's; max_edges: the most ridge edges the caller is prepared to
 *                                   hold records for (40 bytes each while the compute runs), 0: no limit below 2^31 - 1. A ridge
 *                                   of more edges fails with "lbmdem_clearance_compute: the ridge has %llu edges, max_edges is
 *                                   %ld" and leaves no result. counts10. Synchronises; changes nothing a later step reads.
 *   lbmdem_download_clearance       d2[lx][ly] and owner[lx][ly]; either may be NULL, not both
 *   lbmdem_clearance_device         the two planes where they lie on the device, node (x, y) at x * *sy + y (for a torch view);
 *                                   the pad columns ly .. *sy - 1 hold 0 (d2) and -1 (owner); good until the next compute or
 *                                   lbmdem_destroy
 *   lbmdem_download_clearance_hist  the histogram, kmax + 1 longs; cap = 0 leaves `hist` alone and reports *count; a buffer of
 *                                   fewer than *count entries is refused with *count set and nothing written
 *   lbmdem_download_clearance_owners, lbmdem_clearance_owners_device   owned [n + 1] longs and d2max [n + 1] ints, on the host and
 *                                   as device pointers; any pointer may be NULL
 *   lbmdem_download_throats         the table; sized as lbmdem_download_pores is: cap = 0 reports *count, a short buffer is
 *                                   refused ("there are %ld throats, the buffer holds %ld") with *count set and nothing written
 *   These readers are refused, with LBMDEM_EINVAL and "%s: no lbmdem_clearance_compute has been made for the map as it is now",
 *   until a compute has been made, after a refused compute, and after anything the pore readers are refused after: any kind of
 *   step or sub-step, lbmdem_upload_f, lbmdem_upload_kinematics.
 *   lbmdem_write_clearance_files    host only, no handle, no device. In <dir>: throats%.6i.dat -- "# lx %d ly %d n %d\n",
 *                                   "# lo hi edges c_min node\n", then per entry "%d %d %d %d %d\n"; clearance_hist%.6i.dat --
 *                                   "# k nodes\n", then nhist lines "%ld %ld\n" of k and hist[k]; clearance_owners%.6i.dat --
 *                                   "# owner owned d2max\n", then n + 1 lines "%d %ld %d\n"; clearance.data -- one line appended,
 *                                   "%le" of t and " %ld" of each of the ten counts; when the file is created, first the line
 *                                   "# t fluid_nodes d2_max d2_max_node sum_d2 ridge_edges throats grain_throats narrowest_c
 *                                   ownerless_grains kmax"; clearance%.6i.vtk, only when plane != 0 -- legacy STRUCTURED_POINTS
 *                                   on the frames' mesh, lbmdem_write_pore_files' header with the title "lbmdem pore clearance"
 *                                   up to "POINT_DATA %ld\n", then twice, for d2 and for owner: "SCALARS d2 int 1\nLOOKUP_TABLE
 *                                   default\n" ("SCALARS owner int 1 .."), the plane as big-endian 32-bit integers, x fastest,
 *                                   and "\n". It checks fopen ("cannot open"); a negative d2, an owner outside [0, n] and table
 *                                   entries that do not ascend by (lo, hi) with 0 <= lo < hi <= n are refused before anything is
 *                                   written. d2 and owner may be NULL when plane == 0, table when ntable == 0.
 *   lbmdem_write_clearance          the compute on the handle's map (max_edges 0), the downloads, then that formatter with
 *                                   t = nbsteps * dt
 *   lbmdem_set_clearance_output     on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_clearance(dir, nFile, plane) at
 *                                   every DEM event, behind the pore files. Off by default; a checkpoint does not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL: null arguments; a side above 32768; max_edges outside 0 .. 2^31 - 1; a strip of a
 * decomposition or distributed grains (and lbmdem_dist_enable with the setting on); the single-precision library (the host-only
 * formatter exists there too); a directory that cannot be written. */
typedef struct lbmdem_throat {
  int lo, hi, edges, c_min, node;
} lbmdem_throat;
#define LBMDEM_CLEARANCE_COUNTS 10
int lbmdem_clearance_compute(lbmdem_handle* h, const int* map /* NULL: the handle's */, long max_edges, long* counts10);
int lbmdem_download_clearance(lbmdem_handle* h, int* d2, int* owner);   /* [lx][ly], host layout; either may be NULL */
int lbmdem_clearance_device(lbmdem_handle* h, const int** d2, const int** owner, int* sy);   /* device layout, pitch sy */
int lbmdem_download_clearance_hist(lbmdem_handle* h, long* hist, long cap, long* count);
int lbmdem_download_clearance_owners(lbmdem_handle* h, long* owned, int* d2max);   /* [n + 1]; any may be NULL */
int lbmdem_clearance_owners_device(lbmdem_handle* h, const long** owned, const int** d2max);
int lbmdem_download_throats(lbmdem_handle* h, lbmdem_throat* out, long cap, long* count);
int lbmdem_write_clearance(lbmdem_handle* h, const char* dir, int nfile, int plane);
int lbmdem_set_clearance_output(lbmdem_handle* h, int on, int plane);   /* 0: off (default) */
int lbmdem_write_clearance_files(const char* dir, int nfile, int lx, int ly, int plane, const int* d2, const int* owner,
                                 const lbmdem_throat* table, long ntable, const long* hist, long nhist, int n, const long* owned,
                                 const int* d2max, const long* counts10, double t);   /* host only */
/* Pore network: WHICH pores are there, and how are they joined? The pore bodies (the wide places), the constrictions between them,
 * how many neighbours a pore has and how large the constriction is that a front must pass -- the graph that permeability
 * estimates, invasion percolation and clogging studies start from. It is a watershed of the clearance analysis' d2: every fluid
 * node climbs to the local maximum of d2 it belongs to. Every result is an integer and every tie has a rule, so nothing depends on
 * the algorithm; a numpy restatement reproduces everything exactly (tests/network_util.py).
 * Input, as of the call: the map M, lbmdem_download_obst's [lx][ly] or a caller's map of that shape, validated as
 * lbmdem_clearance_compute validates it (the sentence under this function's name); behind it that analysis' d2. Node (x, y) has
 * the index k = x*ly + y, N = lx*ly. Two nodes are ADJACENT when they differ by at most 1 in both x and y (8 neighbours: a
 * diagonal step between two solid corners counts). p is HIGHER than q, p > q below, when d2[p] > d2[q], or d2[p] == d2[q] and
 * p < q: a strict total order on the fluid nodes.
 * 1. Ascent. up(p) is the highest node among p and its adjacent fluid nodes. A fluid node with up(p) == p is a peak; peak(p) is
 *    where repeated up ends (up(p) > p off the peaks).
 * 2. Bodies. The peaks are numbered 0 .. B-1 ascending by node index. body[x][y], int: the number of peak(p), -1 off the fluid.
 *    lbmdem_net_body: node, the peak's index; d2, the peak's d2, the body's largest; nodes, long; degree, the number of level-0
 *    links it is in; parent and group, rule 4.
 * 3. Links, level 0. An edge is a pair of adjacent fluid nodes p < q with different bodies -- q one of p + 1, p + ly - 1, p + ly,
 *    p + ly + 1, inside the lattice and in the same or the next row as adjacency demands. Its height is min(d2[p], d2[q]). One
 *    lbmdem_net_link per distinct pair (lo, hi), lo < hi, of bodies, ascending by (lo, hi): edges; saddle, the largest height
 *    among the pair's edges; node, the smallest p among the edges of that height.
 * 4. Merge, parameter merge (int). merge == -1: parent[a] = a for all a. merge >= 0: the candidates of body a are its links
 *    whose partner b has a peak higher than a's and isqrt(d2 of a's peak) - isqrt(saddle) <= merge, isqrt rounded down as in the
 *    clearance block. parent[a] is the candidate with the largest saddle, among equal saddles the smaller b; without a
 *    candidate a. group[a] is where repeated parent ends (parents are strictly higher: no cycle). ONE round by definition,
 *    not iterated after merging. group[x][y], int: group[body[x][y]], -1 off the fluid.
 * 5. Groups. One lbmdem_net_group per root, ascending by body number: body, the root's number; bodies; nodes, long; d2 and
 *    node, the root's; degree, its level-1 links.
 * 6. Links, level 1: rule 3 with group in place of body; lo and hi are root body numbers.
 * 7. counts10, in order: fluid_nodes; bodies; body_links; body_edges; groups; group_links; group_edges; isolated_groups
 *    (degree 0); largest_group_nodes; narrowest_saddle, the smallest level-1 saddle, -1 without a link.
 * Identities: the bodies' nodes sum to fluid_nodes; with merge == -1 level 1 equals level 0; a map without solid nodes has one
 * body; no body or group spans two 8-connected pores -- every lbmdem_pore_compute(conn 8) component is a union of groups; a link's
 * saddle is at most both peaks' d2.
 * On the device (lbm_network.hip), on the handle's stream, single launches: the clearance compute first where it is needed --
 * with map == NULL and a clearance result of the handle's map that its guard still calls valid, that result's d2 plane is
 * reused; otherwise lbmdem_clearance_compute runs on the map with no edge cap, and its readers are valid afterwards as if the
 * caller had called it. Then the ascent over the key d2 << 32 | (N-1-k) in tiles of 16 x 64 nodes with an apron in LDS, chains
 * shortened in LDS and followed across tiles strictly upward; the peaks numbered by count / scan / emit; the nodes per body
 * (lanes that share a body first, LDS, 64-bit integer atomics); per level count / scan / emit of (pair, value) records, two stable
 * radix sorts, a run-length encode, one kernel per run; the merge by an atomic maximum per body over the links' proposals
 * (saddle << 32 | ~partner: the maximum is rule 4's choice) and a walk up the parents. Integer atomics only, no floating point.
 * Planes and block counts come from the handle's pool with the first call, the tables grow with their counts, the sort's records
 * (40 bytes an edge) live for the call.
 *   lbmdem_network_compute          the compute; map NULL: the handle's; merge: rule 4; max_edges: the most level-0 edges the
 *                                   caller is prepared to hold records for, 0: no limit below 2^31 - 1. More edges fail with
 *                                   "lbmdem_network_compute: the ridge has %llu edges, max_edges is %ld" and leave no network
 *                                   result. counts10. Synchronises; changes nothing a later step reads.
 *   lbmdem_download_network         body[lx][ly] and group[lx][ly]; either may be NULL, not both
 *   lbmdem_network_device           the two planes where they lie on the device, node (x, y) at x * *sy + y (for a torch view);
 *                                   the pad columns ly .. *sy - 1 hold -1; good until the next compute or lbmdem_destroy
 *   lbmdem_download_network_bodies, lbmdem_download_network_groups, lbmdem_download_network_links (level 0 or 1)   the tables;
 *                                   sized as lbmdem_download_throats is: cap = 0 reports *count, a short buffer is refused
 *                                   ("%s: there are %ld bodies (groups, links), the buffer holds %ld") with *count set and
 *                                   nothing written
 *   These readers are refused, with LBMDEM_EINVAL and "%s: no lbmdem_network_compute has been made for the map as it is now",
 *   until a compute has been made, after a refused compute, and after anything the clearance readers are refused after.
 *   lbmdem_write_network_files      host only, no handle, no device. In <dir>: network_bodies%.6i.dat -- "# lx %d ly %d n %d
 *                                   merge %d\n", "# body node d2 nodes degree parent group\n", then per body "%ld %d %d %ld %d
 *                                   %d %d\n"; network_links%.6i.dat -- the same first line, "# lo hi edges saddle node\n", then
 *                                   per link of the table given (lbmdem_write_network gives level 1) "%d %d %d %d %d\n";
 *                                   network_groups%.6i.dat -- the same first line, "# body bodies nodes d2 node degree\n", then
 *                                   per group "%d %d %ld %d %d %d\n"; network.data -- one line appended, "%le" of t and " %ld"
 *                                   of each of the ten counts; when the file is created, first the line "# t fluid_nodes bodies
 *                                   body_links body_edges groups group_links group_edges isolated_groups largest_group_nodes
 *                                   narrowest_saddle"; network%.6i.vtk, only when plane != 0 -- lbmdem_write_clearance_files'
 *                                   layout with the title "lbmdem pore network" and the planes "body" and "group". It checks
 *                                   fopen ("cannot open"); refused before anything is written: bodies whose nodes, groups whose
 *                                   bodies and links whose pairs do not ascend; lo >= hi; a body's group, a group's body or a
 *                                   link's end that is not a root; a negative d2; a plane value outside -1 .. nbodies - 1.
 *                                   body and group may be NULL when plane == 0, a table when its count is 0.
 *   lbmdem_write_network            the compute on the handle's map (max_edges 0), the downloads, then that formatter with the
 *                                   level-1 links and t = nbsteps * dt
 *   lbmdem_set_network_output       on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_network(dir, nFile, merge, plane)
 *                                   at every DEM event, behind the clearance files. Off by default; a checkpoint does not
 *                                   carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL: null arguments; merge < -1; level outside 0 and 1; a side above 32768; max_edges
 * outside 0 .. 2^31 - 1; a strip of a decomposition or distributed grains (and lbmdem_dist_enable with the setting on); the
 * single-precision library (the host-only formatter exists there too); a directory that cannot be written. */
typedef struct lbmdem_net_body {
  int node, d2;
  long nodes;
  int degree, parent, group;
} lbmdem_net_body;
typedef struct lbmdem_net_link {
  int lo, hi, edges, saddle, node;
} lbmdem_net_link;
typedef struct lbmdem_net_group {
  int body, bodies;
  long nodes;
  int d2, node, degree;
} lbmdem_net_group;
#define LBMDEM_NETWORK_COUNTS 10
int lbmdem_network_compute(lbmdem_handle* h, const int* map /* NULL: the handle's */, int merge, long max_edges, long* counts10);
int lbmdem_download_network(lbmdem_handle* h, int* body, int* group);   /* [lx][ly], host layout; either may be NULL, not both */
int lbmdem_network_device(lbmdem_handle* h, const int** body, const int** group, int* sy);   /* device layout, pitch sy */
int lbmdem_download_network_bodies(lbmdem_handle* h, lbmdem_net_body* out, long cap, long* count);
int lbmdem_download_network_groups(lbmdem_handle* h, lbmdem_net_group* out, long cap, long* count);
int lbmdem_download_network_links(lbmdem_handle* h, int level, lbmdem_net_link* out, long cap, long* count);
int lbmdem_write_network(lbmdem_handle* h, const char* dir, int nfile, int merge, int plane);
int lbmdem_set_network_output(lbmdem_handle* h, int on, int merge, int plane);   /* 0: off (default) */
int lbmdem_write_network_files(const char* dir, int nfile, int lx, int ly, int n, int merge, int plane, const int* body,
                               const int* group, const lbmdem_net_body* bodies, long nbodies, const lbmdem_net_group* groups,
                               long ngroups, const lbmdem_net_link* links, long nlinks, const long* counts10, double t);   /* host only */
/* Drainage: how large a particle passes through this packing from the free fluid above it to the base, at what capillary pressure
 * does a non-wetting fluid break through and through which throat, what does a mercury-intrusion curve look like next to the true
 * pore-size distribution? All three are one object: for every fluid node the (squared) size of the largest disc that can be brought
 * there from an inlet side without ever overlapping a solid -- the widest-path value over the clearance analysis' d2. It is an
 * integer and its fixed point is unique whatever the order of evaluation; a numpy restatement over the network and a heap-based
 * widest path over the grid reproduce everything exactly (tests/drainage_util.py).
 * Input, as of the call: the map M, validated as lbmdem_clearance_compute validates it -- the handle's or a caller's of that
 * shape; behind it the clearance's d2 and the pore network's body plane and level-0 link table. Node (x, y) has the index
 * k = x*ly + y. Adjacency is the network's: 8 neighbours, a diagonal step between two solid corners counts.
 * Parameters: from and to, side masks with the walls' bit values: B 1 (y low), T 2 (y high), L 4 (x low), R 8 (x high); band, an int
 * >= 1, each side clamped to the lattice. The REGION of a mask is the set of nodes with y < band (B), y >= ly - band (T), x < band
 * (L) or x >= lx - band (R), for the bits set. (A band is needed because positions outside the lattice count as wall: every edge
 * node has d2 == 1, so a reservoir one node deep admits nothing wider.) The inlet set S is the fluid nodes of from's region, the
 * outlet set T those of to's region. from == 0 is refused; to == 0 is allowed: there is then no outlet.
 * 1. Access. access[x][y], int: for a fluid node p the maximum, over all paths of adjacent fluid nodes from any node of S to p, of
 *    the smallest d2 on the path, both ends included; 0 where no such path exists and 0 off the fluid. So access <= d2, and
 *    access == d2 on S.
 * 2. Per body. A[b], int: the largest access among the body's nodes, 0 if none is reached. It is the least fixed point of
 *    A[b] = max(seed[b], max over level-0 links (b, c) of min(A[c], saddle(b, c))), seed[b] the largest d2 among the nodes of S in
 *    body b, or 0; and access[p] = min(d2[p], A[body[p]]). Why: every node climbs to its peak along non-decreasing d2 and the way
 *    back down is the same nodes, so a path may always be led over the peaks of the bodies it visits without lowering its smallest
 *    d2; and the best crossing between two adjacent bodies, peak to peak, has the link's saddle as its smallest d2.
 * 3. Per level-0 link. pass, int: min(A[lo], A[hi], saddle), the largest size that crosses this link coming from the inlet.
 * 4. Intrusion curve. hist[k], long, k = 0 .. kmax, kmax the clearance block's: the fluid nodes with isqrt(access) == k; hist[0]
 *    is the unreached fluid. It lies next to lbmdem_download_clearance_hist's array entry for entry; the shift between the two is
 *    the ink-bottle effect.
 * 5. counts10, in order: fluid_nodes; inlet_nodes; reached_nodes (access > 0); reached_bodies (A > 0); access_max;
 *    shielded_nodes (0 < access < d2); outlet_nodes; critical, the largest access over T, 0 when T is not reached or empty, -1
 *    when to == 0; critical_node, the smallest index of T with that access and access > 0, otherwise -1; front_links, the level-0
 *    links with saddle == critical, max(A[lo], A[hi]) > critical and min(A[lo], A[hi]) == critical, counted only when
 *    critical > 0: the candidate bottleneck throats. An empty S is not an error: everything is then 0 or -1 as stated.
 * Identities: sum(hist) == fluid_nodes; hist[0] == fluid_nodes - reached_nodes; from == 15 with band >= max(lx, ly) gives
 * access == d2; the nodes of an 8-connected pore (lbmdem_pore_compute, conn 8) without an inlet node have access 0;
 * critical <= access_max; swapping from and to gives the same critical whenever both are non-zero.
 * On the device (lbm_drainage.hip), on the handle's stream: the network first where it is needed -- with map == NULL and a network
 * result of the handle's map that its guard still calls valid (over a clearance result of which the same holds), the body plane,
 * the level-0 link table and d2 are reused, whatever merge that result was made with; otherwise lbmdem_network_compute(map, merge
 * -1, max_edges) runs, and its readers are valid afterwards as if the caller had called it. Then the seed by an atomic maximum
 * per inlet node; the relaxation over the link table in rounds -- a workgroup sweeps its 256 consecutive links until 32 sweeps in
 * a row raised nothing, the host reads a `changed` word and stops at the first quiet launch, at most bodies + 1 launches ("the
 * relaxation did not settle" beyond); no workgroup waits for another; A goes through relaxed agent-scope atomics --; one pass
 * over the plane for access, the histogram (lanes that share a bin first, LDS, 64-bit integer atomics), the node counts and
 * critical (an atomic maximum of access << 32 | ~k over the outlet); one lane per body and link for the rest. Integer atomics
 * only, no floating point. The plane comes from the handle's pool with the first call, the tables grow with their counts.
 *   lbmdem_drainage_compute         the compute; map NULL: the handle's; max_edges: lbmdem_network_compute's, where that runs.
 *                                   counts10. A refused compute leaves no drainage result. Synchronises; changes nothing a
 *                                   later step reads.
 *   lbmdem_download_drainage        access[lx][ly]
 *   lbmdem_drainage_device          the plane where it lies on the device, node (x, y) at x * *sy + y (for a torch view); the pad
 *                                   columns ly .. *sy - 1 hold 0; good until the next compute or lbmdem_destroy
 *   lbmdem_download_drainage_bodies, lbmdem_download_drainage_links   A and pass, aligned with lbmdem_download_network_bodies
 *                                   and lbmdem_download_network_links(level 0); lbmdem_download_drainage_hist: kmax + 1 bins. Sized
 *                                   as lbmdem_download_throats is: cap = 0 reports *count, a short buffer is refused ("%s: there
 *                                   are %ld bodies (links, bins), the buffer holds %ld") with *count set and nothing written
 *   lbmdem_drainage_rounds          the launches of the relaxation in the last compute, the quiet last one included; 0 without
 *                                   a link
 *   These readers are refused, with LBMDEM_EINVAL and "%s: no lbmdem_drainage_compute has been made for the map as it is now",
 *   until a compute has been made, after a refused compute, after anything the network readers are refused after, and after a
 *   later lbmdem_network_compute (the tables A and pass are aligned with are gone).
 *   lbmdem_write_drainage_files     host only, no handle, no device. In <dir>: drainage_curve%.6i.dat -- "# lx %d ly %d n %d from
 *                                   %d band %d to %d\n", "# k access_nodes clearance_nodes invaded\n", then per k = 0 .. kmax "%ld
 *                                   %ld %ld %ld\n": k, hist[k], clearance_hist[k] and the nodes with isqrt(access) >= max(k, 1);
 *                                   drainage_bodies%.6i.dat -- the same first line, "# body node d2 A\n", then per body "%ld %d
 *                                   %d %d\n"; drainage.data -- one line appended, "%le" of t and " %ld" of each of the ten
 *                                   counts; when the file is created, first the line "# t fluid_nodes inlet_nodes reached_nodes
 *                                   reached_bodies access_max shielded_nodes outlet_nodes critical critical_node front_links";
 *                                   drainage%.6i.vtk, only when plane != 0 -- lbmdem_write_clearance_files' layout with the title
 *                                   "lbmdem drainage" and the one plane "access". It checks fopen ("cannot open"); refused
 *                                   before anything is written: nA != nbodies, histograms of different lengths, bodies whose
 *                                   nodes do not ascend, a negative d2, A, count or plane value, A above the body's d2, from,
 *                                   band or to outside their ranges. access may be NULL when plane == 0, bodies and A when
 *                                   their count is 0.
 *   lbmdem_write_drainage           the compute on the handle's map (max_edges 0), the downloads, then that formatter with
 *                                   t = nbsteps * dt
 *   lbmdem_set_drainage_output      on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_drainage(dir, nFile, from, band,
 *                                   to, plane) at every DEM event, behind the network files. Off by default; a checkpoint does
 *                                   not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL: null arguments; from outside 1 .. 15; to outside 0 .. 15; band < 1; a side above
 * 32768; max_edges outside 0 .. 2^31 - 1; a strip of a decomposition or distributed grains (and lbmdem_dist_enable with the
 * setting on); the single-precision library (the host-only formatter exists there too); a directory that cannot be written. */
#define LBMDEM_DRAINAGE_COUNTS 10
int lbmdem_drainage_compute(lbmdem_handle* h, const int* map /* NULL: the handle's */, int from, int band, int to, long max_edges,
                            long* counts10);
int lbmdem_download_drainage(lbmdem_handle* h, int* access);   /* [lx][ly], host layout */
int lbmdem_drainage_device(lbmdem_handle* h, const int** access, int* sy);   /* device layout, pitch sy */
int lbmdem_download_drainage_bodies(lbmdem_handle* h, int* A, long cap, long* count);
int lbmdem_download_drainage_links(lbmdem_handle* h, int* pass, long cap, long* count);
int lbmdem_download_drainage_hist(lbmdem_handle* h, long* hist, long cap, long* count);
int lbmdem_drainage_rounds(lbmdem_handle* h, int* rounds);
int lbmdem_write_drainage(lbmdem_handle* h, const char* dir, int nfile, int from, int band, int to, int plane);
int lbmdem_set_drainage_output(lbmdem_handle* h, int on, int from, int band, int to, int plane);   /* 0: off (default) */
int lbmdem_write_drainage_files(const char* dir, int nfile, int lx, int ly, int n, int from, int band, int to, int plane,
                                const int* access, const lbmdem_net_body* bodies, long nbodies, const int* A, long nA,
                                const long* hist, long nhist, const long* clearance_hist, long nclearance_hist,
                                const long* counts10, double t);   /* host only */
/* Geodesic: how LONG is the way through this packing? Every analysis above says how wide the pore space is; the tortuosity, the
 * ratio of the shortest path through the pores to the straight distance, is the geometric number Kozeny-Carman needs next to the
 * porosity and the wetted surface, and it explains a breakthrough time of the dye or the tracers. For every passable fluid node
 * the length of the shortest path of adjacent passable nodes from an inlet region; on request the same from an outlet region, and
 * from the two the corridor of shortest paths between them. Integers only, and the result is unique whatever the order of
 * evaluation; a numpy restatement by Jacobi sweeps and a heap Dijkstra over the grid reproduce everything exactly
 * (tests/geodesic_util.py).
 * Input, as of the call: the map M, validated as lbmdem_clearance_compute validates it -- the handle's or a caller's of that
 * shape. Node (x, y) has the index k = x*ly + y.
 * Parameters: from and to, side masks as in the drainage block: B 1 (y low), T 2 (y high), L 4 (x low), R 8 (x high); from is
 * non-zero, to == 0 means no outlet; band, an int >= 1, each side clamped to the lattice; the REGION of a mask and band is the
 * drainage block's. conn, 4 or 8. min_d2, an int >= 0.
 * 1. Passable. A fluid node (M == -1) whose clearance d2 (the clearance block's) is >= min_d2. With min_d2 <= 1 this is every
 *    fluid node; the clearance analysis is then neither needed nor run and its result, if there is one, is not touched. With
 *    min_d2 > 1 it is the pore space as a particle of that squared radius sees it.
 * 2. Metric. A step between two passable nodes that differ by 1 in x or in y costs LBMDEM_GEO_UNIT = 5; with conn == 8 a step
 *    between two passable nodes that differ by 1 in both costs 7, whatever the other two nodes of the square are (as the pores'
 *    8-connectivity has it): the 5-7 chamfer, 1.4 against sqrt(2). The unit is a fifth of a node spacing in both modes.
 * 3. dist[x][y], int: 0 on the passable nodes of the region of (from, band); elsewhere the least cost of a path of such steps from
 *    them; -1 where the node is not passable or not reached.
 * 4. back[x][y], int: the same from the passable nodes of the region of (to, band); all -1 when to == 0.
 * 5. shortest: the least dist over the passable nodes of the outlet region, -1 without one (to == 0, an empty outlet, none
 *    reached). detour[x][y], int: dist + back - shortest where both are >= 0 and shortest >= 0, else -1. detour == 0 marks the
 *    nodes that lie on some shortest path from the inlet to the outlet; detour is never negative.
 * 6. Profile. depth(p) is the least offset of p to a side in from: B y, T ly-1-y, L x, R lx-1-x. One lbmdem_geo_level per depth
 *    0 .. depthmax, depthmax the largest depth on the lattice (a matter of lx, ly and from alone): nodes, the passable nodes of
 *    that depth; reached, those with dist >= 0; sum, the sum of dist over them; dmin and dmax, the least and the largest dist
 *    among them, -1 without one. sum / (5 * reached * (depth - band + 1)) is the mean tortuosity at that depth.
 * 7. counts10, in order: fluid_nodes; passable_nodes; inlet_nodes, the passable nodes of from's region; reached_nodes
 *    (dist >= 0); dist_max, -1 when nothing is reached; outlet_nodes, the passable nodes of to's region, 0 when to == 0;
 *    outlet_reached, those with dist >= 0; shortest; shortest_node, the smallest index k among the outlet nodes with
 *    dist == shortest, -1 without one; path_nodes, the nodes with detour == 0.
 * Identities: with conn == 4, dist is 5 times the number of steps of a breadth-first search; dist with conn == 8 is at most dist
 * with conn == 4, node for node; a larger min_d2 never lowers a distance; swapping from and to gives the same shortest; a band
 * that covers the lattice gives dist == 0 on every passable node; sum over the profile's nodes == passable_nodes.
 * On the device (lbm_geodesic.hip), on the handle's stream: with min_d2 > 1 the clearance first where it is needed -- with
 * map == NULL and a clearance result of the handle's map that its guard still calls valid, that result's d2 plane is reused;
 * otherwise lbmdem_clearance_compute runs on the map with max_edges passed through, and its readers are valid afterwards as if the
 * caller had called it. The distances are the greatest fixed point below the seed of D[p] = min(D[p], D[q] + cost(p, q)): values
 * only fall, and only to values a real path realises, so any order of relaxations ends at the same plane. One pass seeds the plane
 * and counts; then rounds over a list of active tiles of 16 x 64 nodes -- a workgroup holds its tile and an apron of one node in
 * LDS, sweeps until a sweep lowers nothing (128 sweeps at most), stores what it lowered and lists for the next round every
 * neighbouring tile that shares a border node it lowered, and itself if it stopped at the bound; the host reads the length of the
 * next list after every launch and stops at the first launch that lists nothing, after passable_nodes + 2 launches at the latest
 * ("the relaxation did not settle" beyond); no workgroup waits for another. The backward pass is the same with the outlet region
 * as seed. One pass for the counts, shortest (an atomic minimum of dist << 32 | k over the outlet) and the profile (LDS bins per
 * depth, then 64-bit integer atomics), one for detour. Integer atomics only, no floating point. The planes come from the handle's
 * pool with the first call.
 *   lbmdem_geodesic_compute         the compute; map NULL: the handle's; max_edges: lbmdem_clearance_compute's, where that runs.
 *                                   counts10. A refused compute leaves no geodesic result. Synchronises; changes nothing a later
 *                                   step reads.
 *   lbmdem_download_geodesic        dist[lx][ly], back[lx][ly], detour[lx][ly]; any pointer may be NULL
 *   lbmdem_geodesic_device          the three planes where they lie on the device, node (x, y) at x * *sy + y (for a torch view);
 *                                   the pad columns ly .. *sy - 1 hold -1; good until the next compute or lbmdem_destroy
 *   lbmdem_download_geodesic_profile   the records; sized as lbmdem_download_throats is: cap = 0 reports *count, a short buffer is
 *                                   refused ("%s: there are %ld depths, the buffer holds %ld") with *count set and nothing written
 *   lbmdem_geodesic_rounds          the launches of the forward and of the backward relaxation in the last compute, the quiet
 *                                   last one included; 0 where the region holds no passable node, *bwd 0 when to == 0
 *   These readers are refused, with LBMDEM_EINVAL and "%s: no lbmdem_geodesic_compute has been made for the map as it is now",
 *   until a compute has been made, after a refused compute, after anything the pore readers are refused after (a step or
 *   sub-step, lbmdem_upload_f, lbmdem_upload_kinematics) and, for a result made with min_d2 > 1 over the handle's map, after a
 *   later lbmdem_clearance_compute (the d2 it was made over is gone).
 *   lbmdem_write_geodesic_files     host only, no handle, no device. In <dir>: geodesic_profile%.6i.dat -- "# lx %d ly %d n %d
 *                                   from %d band %d to %d conn %d min_d2 %d\n", "# depth nodes reached sum min max tortuosity\n",
 *                                   then per depth "%ld %ld %ld %ld %d %d %.6f\n", the last column (double)sum / (double)(5 *
 *                                   reached * (depth - band + 1)), the product formed in 64-bit integers, followed by one
 *                                   division; 0.000000 for depth < band or reached == 0; geodesic.data -- one line appended,
 *                                   "%le" of t and " %ld" of each of the ten counts; when the file is created, first the line
 *                                   "# t fluid_nodes passable_nodes inlet_nodes reached_nodes dist_max outlet_nodes
 *                                   outlet_reached shortest shortest_node path_nodes"; geodesic%.6i.vtk, only when plane != 0 --
 *                                   lbmdem_write_clearance_files' layout with the title "lbmdem geodesic" and the planes "dist",
 *                                   "back" and "detour". It checks fopen ("cannot open"); refused before anything is written:
 *                                   no level, a level with reached > nodes, a negative count or sum, dmin and dmax that are not
 *                                   -1 without a reached node or do not ascend with one, a plane value below -1, from, band, to,
 *                                   conn or min_d2 outside their ranges. The planes may be NULL when plane == 0.
 *   lbmdem_write_geodesic           the compute on the handle's map (max_edges 0), the downloads, then that formatter with
 *                                   t = nbsteps * dt
 *   lbmdem_set_geodesic_output      on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_geodesic(dir, nFile, from, band,
 *                                   to, conn, min_d2, plane) at every DEM event, behind the drainage files. Off by default; a
 *                                   checkpoint does not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL, each with its sentence under the entry point's name: "from must be a mask of sides,
 * B 1 | T 2 | L 4 | R 8, with at least one (%d)"; "to must be a mask of sides, B 1 | T 2 | L 4 | R 8, or 0 for no outlet (%d)";
 * "band must be at least 1 node (%d)"; "conn must be 4 or 8 (%d)"; "min_d2 must not be negative (%d)"; "a lattice of %d x %d nodes
 * has a side above %d or more than %d nodes: a distance is a 32-bit integer" (a side above 32768, or 7 * lx * ly > INT_MAX);
 * "max_edges must lie in 0 .. %d (%ld)"; "map[%ld] = %d (node %ld, %ld) is neither -1 (fluid), a grain (0 .. %d) nor the wall
 * (%d)". Also: null arguments; a strip of a decomposition or distributed grains (and lbmdem_dist_enable with the setting on); the
 * single-precision library (the host-only formatter exists there too); a directory that cannot be written. */
#define LBMDEM_GEO_UNIT 5
typedef struct lbmdem_geo_level {
  long nodes, reached, sum;
  int dmin, dmax;
} lbmdem_geo_level;
#define LBMDEM_GEODESIC_COUNTS 10
int lbmdem_geodesic_compute(lbmdem_handle* h, const int* map /* NULL: the handle's */, int from, int band, int to, int conn,
                            int min_d2, long max_edges, long* counts10);
int lbmdem_download_geodesic(lbmdem_handle* h, int* dist, int* back, int* detour);   /* [lx][ly], host layout; any may be NULL */
int lbmdem_geodesic_device(lbmdem_handle* h, const int** dist, const int** back, const int** detour, int* sy);   /* device layout, pitch sy */
int lbmdem_download_geodesic_profile(lbmdem_handle* h, lbmdem_geo_level* rec, long cap, long* count);
int lbmdem_geodesic_rounds(lbmdem_handle* h, int* fwd, int* bwd);
int lbmdem_write_geodesic(lbmdem_handle* h, const char* dir, int nfile, int from, int band, int to, int conn, int min_d2, int plane);
int lbmdem_set_geodesic_output(lbmdem_handle* h, int on, int from, int band, int to, int conn, int min_d2, int plane);   /* 0: off (default) */
int lbmdem_write_geodesic_files(const char* dir, int nfile, int lx, int ly, int n, int from, int band, int to, int conn, int min_d2,
                                int plane, const int* dist, const int* back, const int* detour, const lbmdem_geo_level* levels,
                                long nlevels, const long* counts10, double t);   /* host only */
/* Pore fluxes: where does the fluid actually go? The analyses above are geometry; this one reads the populations. Per throat of the
 * pore network the mass that crossed it in the last streaming step, per pore whether it fills or drains, its throughput (and so its
 * residence time), and per section of the lattice the net mass through it -- the Darcy flux. D2Q9 makes the answer exact: the
 * network's edges are pairs of adjacent fluid nodes p < q with q one of p+1, p+ly-1, p+ly, p+ly+1, which are the four forward
 * lattice directions 8, 5, 6, 7 (their opposites: 4, 1, 2, 3), and the state a download gives is post-streaming, so between two
 * fluid nodes f[q][i] is what left p in the last streaming step and f[p][opp(i)] what left q. Their difference is the mass that
 * crossed the edge, not an interpolated velocity. Every addend is turned into fixed point as the pore table's mass_q32 is, so every
 * sum is an integer that no order of evaluation changes; a numpy restatement and a node-by-node loop reproduce everything exactly
 * (tests/netflux_util.py).
 * Input, as of the call: the map M, validated as lbmdem_clearance_compute validates it -- the handle's (lbmdem_download_obst's) or
 * a caller's of that shape; f, lbmdem_download_f's [lx][ly][9], always the handle's; behind M the pore network at `merge`: the
 * body and group planes and the link table of `level`. Node (x, y) has the index k = x*ly + y; fluid means M == -1. level 0: the
 * regions are the bodies, in the order of lbmdem_download_network_bodies; level 1: the groups, in the order of
 * lbmdem_download_network_groups. The links are lbmdem_download_network_links(level)'s, entry for entry.
 * 1. Edge quantum. For adjacent fluid nodes p < q with q = p + e_i, i in 8, 5, 6, 7 (offsets +1, +ly-1, +ly, +ly+1, inside the
 *    lattice as the network's rule 3 says): phi = f[q][i] - f[p][opp(i)], one IEEE double subtraction, and
 *    Q(p, q) = (long long) rint(phi * 4294967296.0) when phi is finite and |phi| < 2^20; otherwise Q = 0 and the edge is
 *    UNACCUMULATED (the pore table's rule for mass_q32). Q(q, p) = -Q(p, q).
 * 2. Per link, lbmdem_netflux_link, over the link's edges (those whose ends lie in the two regions): flux_q32, Q oriented from
 *    region lo to region hi, +Q(p, q) when p is in lo and -Q(p, q) when p is in hi; exchange_q32, the sum of |Q| -- against
 *    |flux_q32| it shows counterflow within one throat --; edges, their number, which equals the network link's edges.
 * 3. Per region, lbmdem_netflux_region: mass_q32, the sum over the region's nodes of the pore table's rint(rho * 2^32), rho =
 *    f0 + f1 + ... + f8 in that order, under the same finite / 2^20 rule (a node left out is an UNACCUMULATED NODE); net_q32, the
 *    inflow through the region's links, +flux where the region is hi and -flux where it is lo; through_q32, the sum of |flux_q32|
 *    over the region's links: with net == 0 half of it is the throughput and mass / (through / 2) the residence time in fluid
 *    steps. All are wrapping 64-bit integers, as numpy adds them.
 * 4. Section profiles, over ALL edges of adjacent fluid nodes, of one region or not. col[x], x = 0 .. lx-2: the sum of Q(p, q)
 *    over the edges with p in row x and q in row x+1 (three offsets), the net mass through that section towards +x in the last
 *    streaming step. row[y], y = 0 .. ly-2: the same towards +y between columns y and y+1: +Q from the offsets +1 and +ly+1 with p
 *    in column y, -Q from the offset +ly-1 with p in column y+1. Divided by 2^32 and by the section's length (ly or lx nodes) it is
 *    the superficial (Darcy) flux in lattice units, a density times a lattice velocity; times rho_moy * c it is kg / (m^2 s), as the
 *    flow-fields block converts a velocity by c and a density by rho_moy.
 * 5. counts10, in order: fluid_nodes; regions; links; edges, all adjacent fluid pairs; ridge_edges, those between different
 *    regions (the network's body_edges or group_edges); unaccumulated_edges; unaccumulated_nodes; flowing_links, those with
 *    flux_q32 != 0; strongest_link, the index of the largest |flux_q32|, the smallest among equals, -1 without a link;
 *    largest_imbalance, the largest |net_q32| over the regions, 0 without one.
 * Identities: net_q32 summed over the regions is 0; sum(link.edges) == ridge_edges; net_q32[r] equals the node-by-node sum, over
 * the region's nodes and their 8 neighbours in another region, of Q(q -> p); for every row x the sum over its fluid nodes and
 * their 8 fluid neighbours of Q(q -> p) equals col[x-1] - col[x], with col[-1] = col[lx-1] = 0, and likewise for row; with every
 * population of a direction equal across the lattice and to that of the opposite direction (a fluid at rest) every output but
 * mass_q32 and the counts of nodes and edges is 0.
 * On the device (lbm_netflux.hip), on the handle's stream, single launches: the network first where it is needed -- with map ==
 * NULL and a network result of the handle's map, made with the same merge, that its guard still calls valid, the planes and
 * tables are reused; otherwise lbmdem_network_compute(map, merge, max_edges 0) runs, and its readers are valid afterwards as if
 * the caller had called it. Then per body number the first link of its run (the table ascends by (lo, hi)); one pass over the
 * lattice that reads every node's region and, where it is fluid, its nine populations once, 64 lanes along y marching along x
 * with the row in front in registers; the link of a ridge edge by a binary search of its lo's run; one lane per link and region
 * for the rest. Integer atomics only. The profiles come from the handle's pool with the first call, the tables grow with the
 * network's counts.
 *   lbmdem_netflux_compute          the compute; map NULL: the handle's. counts10. A refused compute leaves no result.
 *                                   Synchronises; changes nothing a later step reads.
 *   lbmdem_download_netflux_links, lbmdem_download_netflux_regions   the tables, aligned with lbmdem_download_network_links(level)
 *                                   and with lbmdem_download_network_bodies (level 0) or _groups (level 1). Sized as
 *                                   lbmdem_download_throats is: cap = 0 reports *count, a short buffer is refused ("%s: there are
 *                                   %ld links (regions), the buffer holds %ld") with *count set and nothing written
 *   lbmdem_download_netflux_profile col[lx - 1] and row[ly - 1]; either may be NULL, not both
 *   These readers are refused, with LBMDEM_EINVAL and "%s: no lbmdem_netflux_compute has been made for the map and populations as
 *   they are now", until a compute has been made, after a refused compute, after anything the network readers are refused after
 *   (any kind of step or sub-step -- a DEM sub-step alone included, as for every stage above, although it changes neither the map
 *   nor f --, lbmdem_upload_f or a grain upload), and after a later lbmdem_network_compute, the caller's or one that another
 *   stage's compute ran (the tables the results are aligned with are gone).
 *   lbmdem_write_netflux_files      host only, no handle, no device. In <dir>: netflux_links%.6i.dat -- "# lx %d ly %d n %d merge
 *                                   %d level %d\n", "# lo hi edges saddle flux_q32 exchange_q32\n", then per link "%d %d %ld %d %ld
 *                                   %ld\n"; netflux_regions%.6i.dat -- the same first line, "# region body nodes mass_q32 net_q32
 *                                   through_q32\n", then per region "%ld %d %ld %ld %ld %ld\n", body the region's (root) body number
 *                                   and nodes its node count; netflux_profile%.6i.dat -- the same first line, "# axis index
 *                                   flux_q32\n", then "x %d %ld\n" per col[x] and "y %d %ld\n" per row[y]; netflux.data -- one line
 *                                   appended, "%le" of t and " %ld" of each of the ten counts; when the file is created, first the
 *                                   line "# t fluid_nodes regions links edges ridge_edges unaccumulated_edges unaccumulated_nodes
 *                                   flowing_links strongest_link largest_imbalance". It checks fopen ("cannot open"); refused before
 *                                   anything is written: merge < -1, level outside 0 and 1, links whose pairs do not ascend, a
 *                                   link whose edges differ between the two tables, regions whose bodies do not ascend, a
 *                                   negative node count. The tables may be NULL when their count is 0.
 *   lbmdem_write_netflux            the compute on the handle's map, the downloads, then that formatter with t = nbsteps * dt
 *   lbmdem_set_netflux_output       on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_netflux(dir, nFile, merge, level)
 *                                   at every DEM event, behind the network files. Off by default; a checkpoint does not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL, "<function>: " and: "level must be 0 (between bodies) or 1 (between groups) (%d)";
 * "merge must be -1 (no merging) or a difference of radii >= 0 (%d)"; "a lattice of %d x %d nodes has a side above %d: the squared
 * distances of the network underneath are 32-bit integers"; "map[%ld] = %d (node %ld, %ld) is neither -1 (fluid), a grain (0 .. %d)
 * nor the wall (%d)". Also: null arguments; a strip of a decomposition or distributed grains (and lbmdem_dist_enable with the
 * setting on); the single-precision library (the host-only formatter exists there too); a directory that cannot be written. */
typedef struct lbmdem_netflux_link {
  long flux_q32, exchange_q32, edges;
} lbmdem_netflux_link;
typedef struct lbmdem_netflux_region {
  long mass_q32, net_q32, through_q32;
} lbmdem_netflux_region;
#define LBMDEM_NETFLUX_COUNTS 10
int lbmdem_netflux_compute(lbmdem_handle* h, const int* map /* NULL: the handle's */, int merge, int level, long* counts10);
int lbmdem_download_netflux_links(lbmdem_handle* h, lbmdem_netflux_link* out, long cap, long* count);
int lbmdem_download_netflux_regions(lbmdem_handle* h, lbmdem_netflux_region* out, long cap, long* count);
int lbmdem_download_netflux_profile(lbmdem_handle* h, long* col /* lx - 1 */, long* row /* ly - 1 */);   /* either may be NULL, not both */
int lbmdem_write_netflux(lbmdem_handle* h, const char* dir, int nfile, int merge, int level);
int lbmdem_set_netflux_output(lbmdem_handle* h, int on, int merge, int level);   /* 0: off (default) */
int lbmdem_write_netflux_files(const char* dir, int nfile, int lx, int ly, int n, int merge, int level, const lbmdem_net_link* links,
                               const lbmdem_netflux_link* flux, long nlinks, const int* region_body, const long* region_nodes,
                               const lbmdem_netflux_region* regions, long nregions, const long* col, const long* row,
                               const long* counts10, double t);   /* host only */
/* Network pressures: what does the pore network predict for pressures and flows when a pressure difference is applied across it?
 * Every link gets a conductance from its width, the regions on an inlet side are held at p = 1, those on an outlet side at p = 0,
 * Kirchhoff's equations are solved for the others, and the flow per link and the total are read off: the permeability of the
 * packing from its geometry alone, and per link the prediction that sits next to the pore fluxes' measured flux_q32. The solver is
 * iterative and in floating point, so the contract is the arithmetic itself: every operation below is one IEEE double operation,
 * rounded before the next (the build has -ffp-contract=off), in the order stated; a numpy restatement reproduces every double on
 * the bits (tests/netsolve_util.py), and nothing depends on the order anything happens in or on how the host batches launches.
 * Input, as of the call: the map M, validated as lbmdem_clearance_compute validates it -- the handle's or a caller's of that
 * shape; behind it the pore network at `merge`: the regions of `level` (0: the bodies, in the order of
 * lbmdem_download_network_bodies; 1: the groups, in the order of lbmdem_download_network_groups) and the link table of that level,
 * lbmdem_download_network_links(level)'s, entry for entry. R regions, Lk links; a link's lo and hi below are the places of its two
 * regions in that order (at level 1 the ranks of its two root bodies).
 * Parameters: from, band, to: the drainage block's side masks and REGION rule, from and to both in 1 .. 15, band >= 1; model, 0 or
 * 1; g_user, Lk doubles when model == 1, else NULL; rtol, a double in (0, 1); max_iter >= 0, 0 meaning the number of free regions,
 * at most 100 000 (the number of free regions is CG's bound in exact arithmetic).
 * 1. Fixed regions. A region that holds a fluid node of from's REGION is an INLET, flags 1, p = 1.0; one that holds a fluid node of
 *    to's REGION and no inlet node is an OUTLET, flags 2, p = 0.0; one with both is an inlet and carries 4 as well (SHORTED, flags
 *    5); all others are FREE, flags 0.
 * 2. Conductance g[l], double. Model 0, plane Poiseuille at unit viscosity: w = 2.0 * sqrt((double)saddle); len =
 *    sqrt((double)(dx*dx + dy*dy)) with dx, dy the integer differences of the two regions' peak nodes (node / ly, node % ly: the
 *    node of the body or group record); g = ((w*w)*w) / (12.0*len). Model 1: g[l] = g_user[l], refused unless every value is
 *    finite and > 0 ("g_user[%ld] = %g: a conductance is finite and > 0" names the first offender).
 * 3. Rows. The row of region a is its incident links in ascending link index -- ascending partner number, because the table
 *    ascends by (lo, hi). diag[a]: the chain from +0.0 of g over the row. apply(v)[a] for a free a: diag[a]*v[a] - s, s the chain
 *    from +0.0 over the row of g*v[partner]; apply(v) is 0 at fixed regions, and every vector below is exactly 0 there. b[a] for a
 *    free a: the chain from +0.0 over the row of g where the partner is an inlet; 0 at fixed regions.
 * 4. dot(u, v). t[a] = u[a]*v[a], padded with +0.0 to a multiple of 256; in every block of 256 consecutive entries, for s = 128, 64,
 *    .., 1: t[i] = t[i] + t[i+s] for i < s, the block's value being t[0]; the block values, padded and reduced the same way, until
 *    one value remains (0.0 without a region). At most 256^3 regions: three levels.
 * 5. Jacobi-preconditioned CG from x = 0. r = b; z = r/diag where a is free and diag[a] > 0, else 0; d = z; rz0 = rz = dot(r, z);
 *    tol2 = rtol*rtol. If rz0 == 0: no iteration, status 0. Iteration k = 1, 2, ..: q = apply(d); dq = dot(d, q); if dq is not
 *    finite or <= 0: status 2, stop, x as it was (k - 1 iterations); alpha = rz/dq; x = x + alpha*d; r = r - alpha*q; z as above;
 *    rzn = dot(r, z); if rzn <= tol2*rz0: status 0, stop; if k == max_iter: status 1, stop; beta = rzn/rz; d = z + beta*d;
 *    rz = rzn. (With every g > 0 the matrix of the free regions is symmetric and diagonally dominant with a positive diagonal, and
 *    d is non-zero while rz is: status 2 needs a rounding accident and has not been seen.)
 * 6. Outputs. Per region lbmdem_netsolve_region: p, 1.0, 0.0 or x; net, the chain from +0.0 over the row of the flow INTO the
 *    region, g*(p[partner] - p[a]); flags; degree, the length of the row. Per link lbmdem_netsolve_link: g, and q = g*(p[lo] -
 *    p[hi]). sums4, doubles: Q_in, rule 4's reduction of -net over the inlets, +0.0 elsewhere; Q_out, the same of +net over the
 *    outlets; rz0; the last dot(r, z) formed (rz0 without an iteration). counts10, in order: regions; links; inlet_regions;
 *    outlet_regions; shorted_regions; free_regions; iterations; status; flowing_links (q != 0); strongest_link, the index of the
 *    largest |q|, the smallest among equals, -1 without a link.
 * Identities: fixed regions hold exactly 1.0 or 0.0; a region whose connected component of the network holds no inlet keeps
 * p == 0.0 and its links q == 0.0 exactly -- b, r, z, d and q never leave 0 there; an empty inlet set is not an error: rz0 == 0,
 * everything 0; from == to makes every fixed region a shorted inlet; Q_in and Q_out agree as far as the residual allows.
 * Q_in * L / W, L and W the lattice's extents along and across the flow, is the permeability in units of the conductance model.
 * On the device (lbm_netsolve.hip), on the handle's stream: the network first where it is needed -- the pore fluxes' rule: with
 * map == NULL and a network result of the handle's map, made with the same merge, that its guard still calls valid, it is reused;
 * otherwise lbmdem_network_compute(map, merge, max_edges 0) runs, and its readers are valid afterwards as if the caller had called
 * it. Once per compute: per link its two regions and g; the rows by a stable radix sort of (hi, link) for the partners below a
 * region and the table's own run for those above, every entry placed by two binary searches, no atomics; the flags by an integer
 * atomic OR per node of the two REGIONs; diag and b by one lane per region, serial over its row. An iteration is two launches: in
 * A every workgroup reduces the blocks' parts of rzn by rule 4 itself, makes the stop tests, forms d = z + beta*d for its own
 * regions and on the fly for its rows' partners, q and its part of dq; in B every workgroup reduces the parts of dq, updates x, r,
 * z and leaves its part of rzn. Every workgroup decides from the same bits; lane 0 of workgroup 0 publishes the status, behind
 * which both kernels return at once; the host enqueues 16 iterations and then reads the status word. No workgroup waits for
 * another, no floating-point atomics, no grid-wide barrier. Everything grows with the network's counts in the handle's pool.
 *   lbmdem_netsolve_compute         the compute; map NULL: the handle's. counts10, sums4. A refused compute leaves no result.
 *                                   Synchronises; changes nothing a later step reads.
 *   lbmdem_download_netsolve_regions, lbmdem_download_netsolve_links   the tables, aligned with lbmdem_download_network_bodies
 *                                   (level 0) or _groups (level 1) and with lbmdem_download_network_links(level). Sized as
 *                                   lbmdem_download_throats is: cap = 0 reports *count, a short buffer is refused ("%s: there are
 *                                   %ld regions (links), the buffer holds %ld") with *count set and nothing written
 *   lbmdem_netsolve_rounds          the launches of the iteration in the last compute: two per iteration enqueued, whole batches
 *   These readers are refused, with LBMDEM_EINVAL and "%s: no lbmdem_netsolve_compute has been made for the map as it is now",
 *   until a compute has been made, after a refused compute, after anything the network readers are refused after, and after a
 *   later lbmdem_network_compute (the tables the results are aligned with are gone).
 *   lbmdem_write_netsolve_files     host only, no handle, no device. In <dir>: netsolve_regions%.6i.dat -- "# lx %d ly %d n %d merge
 *                                   %d level %d from %d band %d to %d\n", "# region body flags degree p net\n", then per region "%ld
 *                                   %d %d %d %.17g %.17g\n", body the region's (root) body number; netsolve_links%.6i.dat -- the
 *                                   same first line, "# lo hi saddle g q\n", then per link "%d %d %d %.17g %.17g\n", lo and hi as
 *                                   the network's table has them; netsolve.data -- one line appended, "%le" of t, " %ld" of each
 *                                   of the ten counts and " %.17g" of each of the four sums; when the file is created, first the
 *                                   line "# t regions links inlet_regions outlet_regions shorted_regions free_regions iterations
 *                                   status flowing_links strongest_link Q_in Q_out rz0 rz". It checks fopen ("cannot open");
 *                                   refused before anything is written: merge, level, from, band or to outside their ranges,
 *                                   tables whose lengths disagree, links whose pairs do not ascend, regions whose bodies do not
 *                                   ascend, flags outside 0 .. 7. The tables may be NULL when their count is 0.
 *   lbmdem_write_netsolve           the compute on the handle's map with model 0, the downloads, then that formatter with
 *                                   t = nbsteps * dt
 *   lbmdem_set_netsolve_output      on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_netsolve(dir, nFile, merge, level,
 *                                   from, band, to, rtol, max_iter) at every DEM event, behind the pore flux files. Off by
 *                                   default; a checkpoint does not carry it.
 * Single-domain fp64 handles. LBMDEM_EINVAL, "<function>: " and: the pore fluxes' sentences for level, merge, the lattice's side
 * and the map; the drainage block's for from and band; "to must be a mask of sides, B 1 | T 2 | L 4 | R 8, with at least one
 * (%d)"; "model must be 0 (plane Poiseuille from the saddle) or 1 (the caller's g) (%d)"; "model 1 needs g_user, one conductance
 * per link"; "g_user must be NULL with model 0"; "rtol must lie strictly between 0 and 1 (%g)"; "max_iter must not be negative, 0:
 * the number of free regions (%d)"; more than 256^3 regions. Also: null arguments; a strip of a decomposition or distributed
 * grains (and lbmdem_dist_enable with the setting on); the single-precision library (the host-only formatter exists there too); a
 * directory that cannot be written. */
typedef struct lbmdem_netsolve_region {
  double p, net;
  int flags, degree;
} lbmdem_netsolve_region;
typedef struct lbmdem_netsolve_link {
  double g, q;
} lbmdem_netsolve_link;
#define LBMDEM_NETSOLVE_COUNTS 10
#define LBMDEM_NETSOLVE_SUMS 4
int lbmdem_netsolve_compute(lbmdem_handle* h, const int* map /* NULL: the handle's */, int merge, int level, int from, int band,
                            int to, int model, const double* g_user, double rtol, int max_iter, long* counts10, double* sums4);
int lbmdem_download_netsolve_regions(lbmdem_handle* h, lbmdem_netsolve_region* out, long cap, long* count);
int lbmdem_download_netsolve_links(lbmdem_handle* h, lbmdem_netsolve_link* out, long cap, long* count);
int lbmdem_netsolve_rounds(lbmdem_handle* h, int* rounds);
int lbmdem_write_netsolve(lbmdem_handle* h, const char* dir, int nfile, int merge, int level, int from, int band, int to, double rtol,
                          int max_iter);
int lbmdem_set_netsolve_output(lbmdem_handle* h, int on, int merge, int level, int from, int band, int to, double rtol,
                               int max_iter);   /* 0: off (default) */
int lbmdem_write_netsolve_files(const char* dir, int nfile, int lx, int ly, int n, int merge, int level, int from, int band, int to,
                                const lbmdem_net_link* links, long nlinks, const lbmdem_netsolve_link* solved, long nsolved,
                                const int* region_body, long nbodies, const lbmdem_netsolve_region* regions, long nregions,
                                const long* counts10, const double* sums4, double t);   /* host only */
/* Coarse-grained fields: per cell of cw x ch lattice nodes the sums people plot -- solid fraction, grain momentum, kinetic energy,
 * coordination and moment tensor next to the fluid's mass, momentum and pore pressure over the SAME cells. The reference adds z, the
 * kinetic-energy terms and M11..M22 over the whole packing only (write_DEM, main.c:373-421); it has no routine for this, so the
 * contract is exact arithmetic: every number is a chain of additions in a fixed order, from +0.0, that a serial loop over the
 * downloads named below reproduces bit for bit.
 * The grid: cw, ch >= 1 nodes per cell in x and y; ncx = (lx + cw - 1) / cw, ncy = (ly + ch - 1) / ch; cell (cx, cy) holds the nodes
 * cx*cw <= x < min(lx, (cx+1)*cw), likewise in y (the last cells are cut at the lattice edge). Records come in host order [ncx][ncy],
 * x slow.
 * Node block (nodes .. sum_P), over the map and populations lbmdem_download_obst and lbmdem_download_f show -- what the last
 * fluid step saw, not a rasterisation a run has already made for the coming one: fluid_nodes obst == -1, grain_nodes
 * 0 <= obst < nbgrains, wall_nodes obst == nbgrains, nodes their total. Per fluid node rho = 0. + f0 + .. + f8,
 * jx = 0. + f0*ex[0] + .. + f8*ex[8], jy likewise (lbmdem_download_macro's values), P = (1./3.) * rho_moy * (rho - 1.)
 * (main.c:320, 533); any other node contributes +0.0. Order of additions, two levels: for each x of the cell a chain over its y
 * ascending, then a chain over x ascending of those column sums.
 * Grain block (grains .. sum_fhf3): a grain belongs to the cell of its centre in node coordinates as the rasteriser forms them
 * (main.c:1009-1010), xc = (x1 - Mgx) / dx, yc = (x2 - Mby) / dx with the walls of lbmdem_get_walls: inside iff xc >= 0 && xc < lx
 * && yc >= 0 && yc < ly (false for NaN), then cx = (int)xc / cw, cy = (int)yc / ch. The others belong to no cell and are counted
 * in `outside` (after the first VerletWall the DEM walls lie ten times beyond the lattice). Chains over the cell's grains in
 * ascending grain index of 1., m, m*v1, m*v2, It*v3, 0.5*m*v1*v1, 0.5*m*v2*v2, 0.5*It*v3*v3 (associated as main.c:381-383 writes
 * them) and fhf1, fhf2, fhf3: the state of lbmdem_download_kinematics and lbmdem_download_fhf, m and It of main.c:624-626.
 * Contact block (sum_z .. M22): the same chains over the columns z, p, M11, M12, M21, M22 of lbmdem_download_grain_table when
 * the last sub-step was a table sub-step (that call's own condition); otherwise all six are +0.0 and contacts_valid is 0, which
 * is no error.
 * On the device: lanes along y stage a lattice row's values in LDS and one lane per cell segment adds them serially, a second
 * kernel chains the column sums over x; the grains get their cell as a key, a stable radix sort keeps a cell's grains in index
 * order and one lane per cell walks its segment. No atomics, nothing depends on launch order. Scratch is allocated by the first
 * call and kept until lbmdem_destroy.
 *   lbmdem_coarse_grid         host only, no handle: *ncx, *ncy
 *   lbmdem_coarse_fields       *count = ncx * ncy; cap_cells = 0 (out may be NULL) only reports it; a buffer of fewer cells is
 *                              refused with *count set; info2 = {outside, contacts_valid}; synchronises; changes nothing a later
 *                              step reads
 *   lbmdem_write_coarse_files  host only, no handle, no device: <dir>/coarse%.6i.dat -- "# cw %d ch %d ncx %d ncy %d outside %ld
 *                              contacts %d\n", then per cell, cx outer and cy inner, "%d %d" followed by the 25 members as " %le"
 *                              and "\n". It checks fopen.
 *   lbmdem_write_coarse        the download, then that formatter
 *   lbmdem_set_coarse_output   cw, ch >= 1: lbmdem_run_scene (comm == NULL) calls lbmdem_write_coarse at every DEM event with the
 *                              event's nFile, behind write_DEM / write_forces (queued first where tables go to the background) and
 *                              behind the contact files when those are on. 0, 0: off (the default); a checkpoint does not carry it.
 * LBMDEM_EINVAL: cw or ch < 1 (except 0, 0 in the setter); null arguments; a strip of a decomposition or distributed grains (and
 * lbmdem_dist_enable with the setting on); the single-precision library (the two host-only calls work there too); a directory
 * that cannot be written ("cannot open"). Vibrating and probing handles have the export. */
typedef struct lbmdem_coarse_cell {
  double nodes, fluid_nodes, grain_nodes, wall_nodes;
  double sum_rho, sum_jx, sum_jy, sum_P;
  double grains, sum_m, sum_mv1, sum_mv2, sum_Iw, ke_x, ke_y, ke_teta;
  double sum_fhf1, sum_fhf2, sum_fhf3;
  double sum_z, sum_p, M11, M12, M21, M22;
} lbmdem_coarse_cell;
#define LBMDEM_COARSE_DOUBLES 25
int lbmdem_coarse_grid(int lx, int ly, int cw, int ch, int* ncx, int* ncy);   /* host only */
int lbmdem_coarse_fields(lbmdem_handle* h, int cw, int ch, lbmdem_coarse_cell* out, long cap_cells, long* count, long* info2);
int lbmdem_write_coarse(lbmdem_handle* h, const char* dir, int nfile, int cw, int ch);
int lbmdem_write_coarse_files(const char* dir, int nfile, int lx, int ly, int cw, int ch, const lbmdem_coarse_cell* cells,
                              long outside, int contacts_valid);   /* host only */
int lbmdem_set_coarse_output(lbmdem_handle* h, int cw, int ch);   /* 0, 0: off (default) */
/* Flow fields: what people show of the fluid in a submerged collapse -- the composite velocity of fluid and grains, its vorticity
 * and divergence, the model's own local strain rate (the non-equilibrium stress moments the MRT collision forms at every node and
 * throws away, main.c:1095-1106), the shear rate and the viscous dissipation -- and the fluid's line of the energy budget, made
 * where the state lies. The reference has no such routine, so the contract is exact arithmetic: IEEE double, no contraction, every
 * expression associated as written here; a restatement over the downloads named below reproduces every value bit for bit. Lattice
 * units throughout.
 * Inputs, as of the call: f = lbmdem_download_f, obst = lbmdem_download_obst, x1 x2 v1 v2 v3 = lbmdem_download_kinematics,
 * Mgx Mby = lbmdem_get_walls, dx c s8 s9 nbgrains = lbmdem_get_config. x, y are node indices converted to double.
 * Per node (x, y) with o = obst[x][y] and fq = f[x][y][q]:
 *   fluid (o == -1):        rho = (((((((f0 + f1) + f2) + f3) + f4) + f5) + f6) + f7) + f8          main.c:1082
 *                           jx  = ((((f5 + f6) + f7) - f1) - f2) - f3                                main.c:1091
 *                           jy  = ((((f1 + f8) + f7) - f3) - f4) - f5                                main.c:1093
 *                           pxx = ((f2 - f4) + f6) - f8        pxy = (((-f1) + f3) - f5) + f7        main.c:1095-1096
 *                           ux = jx / rho        uy = jy / rho
 *                           nxx = pxx - ((jx * jx) - (jy * jy)) / rho        nxy = pxy - (jx * jy) / rho      main.c:1105-1106
 *                           D = ((-1.5 * s8) * nxx) / rho        T = ((-3. * s9) * nxy) / rho
 *                           gdot = sqrt((D * D) + (T * T))
 *                           diss = rho * (((nu8 * D) * D) + ((nu9 * T) * T)),  nu8 = ((1. / s8) - 0.5) / 3., nu9 likewise with s9
 *                           (formed once on the host)
 *   grain (0 <= o < nbgrains, i = o): ux = (v1[i] - (((y * dx) + Mby) - x2[i]) * v3[i]) / c            main.c:974
 *                           uy = (v2[i] + (((x * dx) + Mgx) - x1[i]) * v3[i]) / c                    main.c:975
 *                           (the grain's present kinematics and the handle's present walls: a vibrating handle's moved Mgx enters)
 *   anything else (the lattice-edge walls, o == nbgrains, among them): ux = uy = +0.0. A lid's speed (lbmdem_set_lid) is NOT
 *                           represented: the plate's nodes show +0.0.
 *   nxx, nxy, gdot, diss are +0.0 at every node that is not fluid.
 *   For 1 <= x <= lx - 2 and 1 <= y <= ly - 2:
 *                           vort = ((uy[x+1][y] - uy[x-1][y]) * 0.5) - ((ux[x][y+1] - ux[x][y-1]) * 0.5)
 *                           div  = ((ux[x+1][y] - ux[x-1][y]) * 0.5) + ((uy[x][y+1] - uy[x][y-1]) * 0.5)
 *   and +0.0 on the outer ring.
 * D and T are the model's d(ux)/dx - d(uy)/dy and d(uy)/dx + d(ux)/dy: to first order the moments are
 * nxx = -(2 / (3 s8)) rho (dx ux - dy uy) and nxy = -(1 / (3 s9)) rho (dx uy + dy ux); they need no stencil across a grain surface.
 * To SI units: velocities x c (m/s); vort, div, D, T, gdot / dtLB (1/s), dtLB = dx / c (lbmdem_get_config); diss is rho nu S^2 per
 * unit volume with rho in units of rho_moy (kg/m^3), nu in dx^2 / dtLB and the rates in 1 / dtLB, so
 * diss_SI = diss * rho_moy * dx^2 / dtLB^3 = diss * rho_moy * c^3 / dx (W/m^3); a node's kinetic energy 0.5 rho u^2 times
 * rho_moy * c^2 is J/m^3.
 * Planes: every selected field is one [lx][ly] plane of doubles, y fastest (the host layout of obst); the planes follow each other
 * in ascending bit order of the mask. count = (bits set in mask) * lx * ly.
 *   lbmdem_flow_fields          copies the planes to the host. *count is always set; cap_doubles = 0 (out may be NULL) only reports it;
 *                               a buffer of fewer doubles is refused with *count set. Synchronises.
 *   lbmdem_flow_fields_device   writes the same planes into the caller's DEVICE memory (cap_doubles >= count, else refused) on the
 *                               handle's stream and does not synchronise: the route for a torch tensor (data_ptr()); order through
 *                               lbmdem_set_stream or lbmdem_sync.
 *   lbmdem_flow_sums            over the fluid nodes only, sums8 = { n_fluid, sum rho, sum (0.5 * rho) * ((ux * ux) + (uy * uy)),
 *                               sum diss, sum (0.5 * vort) * vort, max ((ux * ux) + (uy * uy)), max gdot, max |div| }. A node that
 *                               is not fluid contributes +0.0. Order of additions, three levels, each a chain from +0.0: per lattice
 *                               row x and block of 64 consecutive y (y / 64; the last block may be short) over y ascending; per row
 *                               over its block sums ascending; over the row sums, x ascending. Maxima start from +0.0 and are
 *                               order-free; n_fluid is an integer in a double. No atomics, nothing depends on launch order.
 *                               Synchronises.
 *   lbmdem_write_flow_files     host only, no handle, no device: <dir>/flow%.6i.vtk from five planes [lx][ly] of doubles -- the
 *                               binary rectilinear-mesh format of the files lbmdem_write_vtk_fields writes (same header, mesh and
 *                               CELL_DATA / POINT_DATA lines, big-endian float, x fastest), then "VECTORS fluid_velocity_lb float\n"
 *                               with (float)ux, (float)uy, 0 per node, and "SCALARS <name> float\nLOOKUP_TABLE default\n" with the
 *                               payload for vorticity (vort), shear_rate (gdot) and dissipation (diss), back to back. lx, ly >= 2.
 *   lbmdem_write_flow           the same file of the handle's present state; the byte image is made on the device.
 *   lbmdem_set_flow_output      on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_flow at every VTK event of a run with
 *                               the fluid, with the event's nFile, after the frame, and at every DEM event, after the existing
 *                               files, appends "%le" of nbsteps * dt and " %le" of the eight sums to <dir>/flow.data (a header line
 *                               "# t n_fluid sum_rho sum_ke sum_diss sum_enstrophy max_u2 max_gdot max_abs_div" when the file is
 *                               created). Synchronous. 0: off (the default); a checkpoint does not carry it.
 * Everything is off by default: nothing is allocated or launched until a call asks for it; scratch comes from the handle's pool and
 * goes with the handle. No call changes anything a later step reads.
 * LBMDEM_EINVAL: a mask of 0 or with bits beyond LBMDEM_FLOW_ALL; null arguments; a short buffer; a strip of a decomposition or
 * distributed grains (and lbmdem_dist_enable with the setting on); the single-precision library (lbmdem_write_flow_files works there
 * too); a directory that cannot be written ("cannot open"). Vibrating, probing and lid handles have the export. */
#define LBMDEM_FLOW_UX 1
#define LBMDEM_FLOW_UY 2
#define LBMDEM_FLOW_VORT 4
#define LBMDEM_FLOW_DIV 8
#define LBMDEM_FLOW_NXX 16
#define LBMDEM_FLOW_NXY 32
#define LBMDEM_FLOW_GDOT 64
#define LBMDEM_FLOW_DISS 128
#define LBMDEM_FLOW_ALL 255
int lbmdem_flow_fields(lbmdem_handle* h, int mask, double* out, long cap_doubles, long* count);
int lbmdem_flow_fields_device(lbmdem_handle* h, int mask, void* dev_out, long cap_doubles);
int lbmdem_flow_sums(lbmdem_handle* h, double* sums8);
int lbmdem_write_flow(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_write_flow_files(const char* dir, int nfile, int lx, int ly, const double* ux, const double* uy, const double* vort,
                            const double* gdot, const double* diss);   /* host only */
int lbmdem_set_flow_output(lbmdem_handle* h, int on);               /* 0: off (default) */
/* Fluid tracers: the Lagrangian view the snapshots above cannot give -- massless particles carried by the composite velocity of
 * fluid and grains, advanced on the device once per fluid step from the velocity field of that step. Pathlines of the pore fluid,
 * of the ambient fluid a collapsing column entrains, of the fluid that rides inside the packing. The reference has no such
 * routine, so the contract is exact arithmetic, as for the flow fields: IEEE double, no contraction, every expression associated
 * as written here; a restatement over the downloads named in the flow-fields block reproduces every position bit for bit.
 * Coordinates: a tracer is (px, py) in node coordinates -- node (x, y) sits at ((double)x, (double)y) -- inside the domain
 * [0, lx - 1] x [0, ly - 1]. Tracer k of the set stays tracer k: nothing sorts or bins them.
 * Velocity at a point (px, py) of the domain, from ux, uy of the flow-fields block (same inputs, same formulas, a lid not
 * represented):
 *   i = (int)px, lowered to lx - 2 if larger;  j = (int)py, lowered to ly - 2 if larger
 *   a = px - i,  b = py - j                    (a may be exactly 1.0 on the last node, likewise b)
 *   w00 = (1. - a) * (1. - b)    w10 = a * (1. - b)    w01 = (1. - a) * b    w11 = a * b
 *   U = (((w00 * ux[i][j]) + (w10 * ux[i+1][j])) + (w01 * ux[i][j+1])) + (w11 * ux[i+1][j+1]),  V likewise from uy
 * One advance is one lattice time unit, a midpoint step in the field as the call finds it:
 *   (U0, V0) at (px, py);   qx = clamp(px + 0.5 * U0), qy = clamp(py + 0.5 * V0);   (U1, V1) at (qx, qy);
 *   px' = clamp(px + U1), py' = clamp(py + V1)
 *   clamp(v) on the x axis is !(v >= 0.) ? 0. : (v > (double)(lx - 1) ? (double)(lx - 1) : v), on the y axis with ly - 1: a NaN
 *   goes to 0 and never reaches an index. (All four nodes of a cell enter with their weight, a weight of 0 included: a node
 *   whose velocity is not finite makes U, V NaN for every point of the cells that touch it.) The lattice-edge walls hold +0.0, so
 *   a midpoint on the last row or column sees no velocity across it.
 * Sample at the present positions, per tracer: U, V as above and o = (double)obst[(int)(px + 0.5)][(int)(py + 0.5)], the nearest
 * node's owner (-1: fluid, 0 .. nbgrains - 1: that grain, nbgrains: a lattice-edge wall).
 *   lbmdem_tracer_set           n tracers from xy = n x (px, py) on the host, replacing an earlier set (whose counts start again);
 *                               n = 0 (xy may be NULL) frees it. The buffers come from the handle's pool and go with the set or
 *                               the handle. automatic != 0: every fluid step advances the set once, on the handle's stream behind
 *                               the force kernels and the probe sample (lbmdem_forces_fluid; so in lbmdem_lbm_step, lbmdem_run,
 *                               lbmdem_run_scene): it sees f after collide_stream, that step's map, and the grains as the sub-step
 *                               before left them -- what a probe sample sees. automatic == 0: only lbmdem_tracer_advance advances.
 *                               A position that is not finite or lies outside the domain is refused, naming the first offender;
 *                               n is at most 2^30 / 40 (positions and the sample's scratch stay under 1 GiB). Synchronises.
 *   lbmdem_tracer_advance       one advance in the present state (f = lbmdem_download_f, obst = lbmdem_download_obst, the present
 *                               kinematics and walls), on the handle's stream; does not synchronise. Nothing to do without tracers.
 *   lbmdem_tracer_download      the positions, n x (px, py). *count is always set; cap = 0 (xy may be NULL) only reports it; a buffer
 *                               of fewer tracers is refused with *count set. Settles and synchronises.
 *   lbmdem_tracer_device        the DEVICE address of the positions ([n][2] doubles, NULL without tracers), for a torch tensor view;
 *                               valid until the next lbmdem_tracer_set. A position written through it is clamped as above when a
 *                               kernel reads it. Order through lbmdem_set_stream or lbmdem_sync.
 *   lbmdem_tracer_sample        out3 = n x (U, V, o) at the present positions; count and cap as for the download. Synchronises.
 *   lbmdem_tracer_stats         counts3 = { tracers, advances made since lbmdem_tracer_set, those of them made by fluid steps }.
 *   lbmdem_write_tracers_files  host only, no handle, no device: <dir>/tracers%.6i.vtk, legacy binary POLYDATA, every number
 *                               big-endian, no separators after binary blocks: "# vtk DataFile Version 2.0\nlbmdem fluid tracers\n
 *                               BINARY\nDATASET POLYDATA\n", "POINTS n float\n" with ((float)px * pas, (float)py * pas, 0) per tracer,
 *                               pas = (float)(1. / lx) -- the coordinates of the frames' mesh, so the file overlays a frame --,
 *                               "VERTICES n 2n\n" with the 32-bit integers (1, k) per tracer, "POINT_DATA n\n",
 *                               "VECTORS tracer_velocity_lb float\n" with ((float)U, (float)V, 0) and "SCALARS tracer_owner float\n
 *                               LOOKUP_TABLE default\n" with (float)o, from xy = n x (px, py) and uvo = n x (U, V, o). n = 0 (the
 *                               buffers may be NULL) writes a valid empty file. lx >= 2.
 *   lbmdem_write_tracers        the same file of the handle's present positions and their sample. Synchronises.
 *   lbmdem_set_tracer_output    on != 0: lbmdem_run_scene (comm == NULL) calls lbmdem_write_tracers at every VTK event of a run with
 *                               the fluid, with the event's nFile, after the frame and the flow file. Synchronous. 0: off (the
 *                               default).
 * Give-up recovery: an advance queued behind a launch of the multi-sub-step DEM kernel that gave up finds the stop word and does
 * nothing; the replay repeats those fluid steps and advances again, once each, and the counts follow.
 * The advance only reads the step's state and writes the tracers' own buffer: no call changes anything a later step reads. With
 * no tracers set nothing is allocated or launched. A checkpoint does not carry tracers or the output setting: a loaded handle has
 * none, and the file is byte for byte what a handle without tracers saves -- unless lbmdem_set_checkpoint_contents has
 * LBMDEM_CKPT_TRACERS on: then the positions and the two counts are in the file and come back with it (never the output setting).
 * LBMDEM_EINVAL: a strip of a decomposition or distributed grains (and lbmdem_dist_enable with tracers set or the output on); the
 * single-precision library (lbmdem_write_tracers_files works there too); null arguments; a short buffer; a bad position or count;
 * a directory that cannot be written ("cannot open"). Vibrating, probing and lid handles have the feature. */
int lbmdem_tracer_set(lbmdem_handle* h, long n, const double* xy, int automatic);
int lbmdem_tracer_advance(lbmdem_handle* h);
int lbmdem_tracer_download(lbmdem_handle* h, double* xy, long cap, long* count);
int lbmdem_tracer_device(lbmdem_handle* h, void** xy);
int lbmdem_tracer_sample(lbmdem_handle* h, double* out3, long cap, long* count);
int lbmdem_tracer_stats(lbmdem_handle* h, long* counts3);
int lbmdem_write_tracers(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_write_tracers_files(const char* dir, int nfile, int lx, long n, const double* xy, const double* uvo);   /* host only */
int lbmdem_set_tracer_output(lbmdem_handle* h, int on);             /* 0: off (default) */
/* Passive scalar: a dye field carried by the fluid's velocity and diffused -- what the snapshots and the tracers cannot show:
 * mixing. How much ambient fluid a collapsing column entrains, how far the pore fluid of the packing spreads, how a dyed layer
 * is stirred. A second lattice of five populations per node, stepped on the device once per fluid step from that step's
 * velocity. The reference has no such routine, so the contract is exact arithmetic, as for the flow fields and the tracers:
 * IEEE double, no contraction, every expression associated as written here; a restatement over the downloads named in the
 * flow-fields block and lbmdem_scalar_download_state reproduces every population bit for bit.
 * State: g_k per node, k = 0..4, on the directions q = 0, 2, 4, 6, 8 of the fluid's set (main.c:70-71):
 *   e_0 = (0, 0), e_1 = (-1, 0), e_2 = (0, -1), e_3 = (1, 0), e_4 = (0, 1);  opp(1) = 3, opp(2) = 4, opp(3) = 1, opp(4) = 2;
 *   w_0 = 1. / 3, w_1 .. w_4 = 1. / 6;  C = (((g_0 + g_1) + g_2) + g_3) + g_4, the concentration;
 *   tau_s > 0.5, the relaxation time given at set time; omega = 1. / tau_s, formed once on the host;
 *   was_fluid, the scalar's own record of the nodes that were fluid when it was last stepped or set. A node outside was_fluid
 *   holds five +0.0, so its C reads +0.0: the field, its sums and its file live on was_fluid.
 * Diffusivity in lattice units D = (tau_s - 0.5) / 3; to SI: D * dx^2 / dtLB = D * dx * c (m^2/s), dtLB = dx / c
 * (lbmdem_get_config). C has the unit the caller gives it.
 * One step, with M = lbmdem_download_obst, f = lbmdem_download_f, the kinematics and walls of the flow-fields block (what a
 * tracer advance sees; a hooked step sees f after this fluid step's collide_stream, that step's map, the grains as the sub-step
 * before left them). For every node n with M[n] == -1, all three stages reading the state as the stage before left it:
 *   1. refill  if n is not in was_fluid (a grain has uncovered it): of the neighbours n + e_1, n + e_2, n + e_3, n + e_4, in that
 *              order, those inside the lattice with M == -1 that are in was_fluid are eligible; S = +0.0, then S = S + C(neighbour)
 *              for each eligible one with its stored C; Cf = S / (double)count, or +0.0 when none is eligible; g_k(n) = w_k * Cf.
 *              Otherwise g_k(n) is the stored value. (Only nodes outside was_fluid are written, only nodes inside it are read.)
 *   2. collide ux, uy of the flow-fields block at n (jx / rho, jy / rho of a fluid node); C = (((g_0 + g_1) + g_2) + g_3) + g_4;
 *              eq_0 = w_0 * C;  eq_k = (w_k * C) * (1. + (3. * s_k)), s_1 = -ux, s_2 = -uy, s_3 = ux, s_4 = uy  (e_k . u);
 *              g*_k = g_k - (omega * (g_k - eq_k))
 *   3. pull    g_k(n) = g*_k(n - e_k) if n - e_k lies inside the lattice and M[n - e_k] == -1, else g*_opp(k)(n): half-way
 *              bounce-back, no flux through grains or the lattice-edge walls. There is NO moving-wall term: a grain that moves
 *              pushes no dye ahead of it through this rule (it does through the refill, below).
 * Every node with M[n] != -1 holds five +0.0 afterwards, and was_fluid becomes M == -1.
 * A node that a grain covers loses its content, and a node that a grain uncovers takes its neighbours' mean: the total of C is NOT
 * conserved where grains move -- the treatment the reference gives the fluid's own mass in reinit_obst_density (main.c:966-986).
 * Where no grain moves the total is conserved to rounding. lbmdem_scalar_sums lets a run watch the drift.
 *   lbmdem_scalar_set             C = [lx][ly] doubles, y fastest: g_k = w_k * C[n] at the fluid nodes of lbmdem_download_obst,
 *                                 five +0.0 elsewhere, was_fluid = that set, replacing an earlier scalar (whose counts start
 *                                 again). Every value of the plane must be finite, those at other nodes (which are ignored)
 *                                 included. C == NULL removes the scalar and frees its buffers (tau_s is not looked at). The
 *                                 buffers -- two sets of five planes, a byte plane, a concentration plane: 89 bytes per node --
 *                                 come from the handle's pool. automatic != 0: every fluid step steps the field once, on the
 *                                 handle's stream behind the force kernels, the probe sample and the tracer advance
 *                                 (lbmdem_forces_fluid; so in lbmdem_lbm_step, lbmdem_run, lbmdem_run_scene). Synchronises.
 *   lbmdem_scalar_step            one step by hand in the present state, on the handle's stream; does not synchronise. Nothing
 *                                 to do without a scalar.
 *   lbmdem_scalar_download        the concentration plane C[lx][ly], +0.0 outside was_fluid. Settles and synchronises.
 *   lbmdem_scalar_download_state  g = [lx][ly][5] and was = [lx][ly] bytes (0 or 1): what a restatement starts from.
 *   lbmdem_scalar_device          the DEVICE address of a concentration plane ([lx][ly] doubles, NULL without a scalar) for a torch
 *                                 tensor view, valid until the next lbmdem_scalar_set. refresh != 0 writes the present field into
 *                                 it on the handle's stream and does not synchronise (order through lbmdem_set_stream or
 *                                 lbmdem_sync); a step does not touch the plane. Writing into it changes nothing of the scalar.
 *   lbmdem_scalar_sums            out5 = { nodes in was_fluid, sum C, sum C * C, min C, max C } over the nodes in was_fluid. Sums:
 *                                 the flow sums' three levels, each a chain from +0.0 -- per lattice row x and block of 64
 *                                 consecutive y over y ascending (a node outside was_fluid adds +0.0), per row over its blocks
 *                                 ascending, over the rows, x ascending. Minimum and maximum are order-free (fmin, fmax from
 *                                 +inf, -inf) and read +0.0 when was_fluid is empty. No atomics. Synchronises.
 *   lbmdem_scalar_stats           counts3 = { 1 if a scalar is set else 0, steps made since lbmdem_scalar_set, those of them made
 *                                 by fluid steps }.
 *   lbmdem_write_scalar_files     host only, no handle, no device: <dir>/scalar%.6i.vtk from C[lx][ly], legacy binary
 *                                 STRUCTURED_POINTS on the nodes of the frames' mesh, so the file overlays a frame:
 *                                 "# vtk DataFile Version 2.0\nlbmdem passive scalar\nBINARY\nDATASET STRUCTURED_POINTS\n",
 *                                 "DIMENSIONS lx ly 1\nORIGIN 0 0 0\nSPACING p p 1\n" with p = "%.9g" of (float)(1. / lx),
 *                                 "POINT_DATA lx*ly\nSCALARS concentration float\nLOOKUP_TABLE default\n", then (float)C of every
 *                                 node, big-endian, x fastest ([ly][lx]), nothing behind it. lx, ly >= 2.
 *   lbmdem_write_scalar           the same file of the handle's present field. Synchronises.
 *   lbmdem_set_scalar_output      on != 0: while a scalar is set lbmdem_run_scene (comm == NULL) calls lbmdem_write_scalar at every
 *                                 VTK event of a run with the fluid, with the event's nFile, after the frame, the flow file and the
 *                                 tracers' file, and at every DEM event, after the existing files, appends "%le" of the step
 *                                 counter nbsteps and " %le" of the five sums to <dir>/scalar.data (a header line
 *                                 "# step n_fluid sum_C sum_C2 min_C max_C" when the file is created). Synchronous. 0: off (the
 *                                 default).
 * Give-up recovery: a step queued behind a launch of the multi-sub-step DEM kernel that gave up finds the stop word and does
 * nothing; the replay repeats those fluid steps and steps the field again, once each, and the counts follow.
 * The step only reads the fluid's state and writes the scalar's own buffers: no call changes anything a later fluid step or DEM
 * sub-step reads. With no scalar set nothing is allocated or launched. A checkpoint does not carry the scalar or the output
 * setting: a loaded handle has none, and the file is byte for byte what a handle without one saves -- unless
 * lbmdem_set_checkpoint_contents has LBMDEM_CKPT_SCALAR on: then the populations, the fluid flags of the last step, tau_s and the
 * counts are in the file and come back with it (never the output setting).
 * LBMDEM_EINVAL: a strip of a decomposition or distributed grains (and lbmdem_dist_enable with a scalar set or the output on); the
 * single-precision library (lbmdem_write_scalar_files works there too); null arguments; tau_s <= 0.5 or not finite; a value of C
 * that is not finite; a download, the sums or the file without a scalar; a directory that cannot be written ("cannot open").
 * Vibrating, probing, lid and tracer handles have the feature. Not built: sources, sinks and Dirichlet nodes during a run, a
 * moving-wall flux term, a scalar that acts back on the fluid, more than one scalar. */
int lbmdem_scalar_set(lbmdem_handle* h, const double* C, double tau_s, int automatic);
int lbmdem_scalar_step(lbmdem_handle* h);
int lbmdem_scalar_download(lbmdem_handle* h, double* C);
int lbmdem_scalar_download_state(lbmdem_handle* h, double* g, unsigned char* was);
int lbmdem_scalar_device(lbmdem_handle* h, void** C, int refresh);
int lbmdem_scalar_sums(lbmdem_handle* h, double* out5);
int lbmdem_scalar_stats(lbmdem_handle* h, long* counts3);
int lbmdem_write_scalar(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_write_scalar_files(const char* dir, int nfile, int lx, int ly, const double* C);   /* host only */
int lbmdem_set_scalar_output(lbmdem_handle* h, int on);             /* 0: off (default) */
/* Time-averaged flow statistics: what a run of this model is reported as -- the mean velocity field of a collapse or a slope
 * flow, the fluctuation energy and the Reynolds shear stress around that mean, the mean density (pore pressure), how much of the
 * time a node lies inside a grain. Every export above is an instant; these are sums over hundreds of fluid steps, accumulated
 * on the device, one pass per sample. The reference has no such routine, so the contract is exact arithmetic, as for the flow
 * fields: IEEE double, no contraction, every expression associated as written here; a restatement over the downloads named in
 * the flow-fields block and lbmdem_mean_download reproduces every accumulator bit for bit.
 * A window is a set of per-node accumulators, all +0.0 / 0 when it opens:
 *   always            n_fluid[x][y], n_grain[x][y]  32-bit unsigned counts;  samples, a count on the host
 *   LBMDEM_MEAN_U     Sux, Suy          a fluid node adds ux, uy
 *   LBMDEM_MEAN_UU    Sxx, Sxy, Syy     a fluid node adds ux * ux, ux * uy, uy * uy (each product rounded, then added)
 *   LBMDEM_MEAN_RHO   Srho, Srho2       a fluid node adds rho, rho * rho
 *   LBMDEM_MEAN_DISS  Sdiss, Sgdot      a fluid node adds diss, gdot
 *   LBMDEM_MEAN_GRAIN Sgux, Sguy        a grain's node adds ux, uy of the composite velocity (the grain's rigid-body velocity)
 * planes of doubles; those outside the window's mask do not exist. rho, ux, uy, gdot, diss are those of the flow-fields block
 * above: same inputs (f, obst, the present kinematics and walls; a hooked sample sees what a probe sample sees), same formulas,
 * a lid not represented.
 * One sample: at every node exactly one of three things happens. o == -1: n_fluid = n_fluid + 1 and S = S + v for every selected
 * fluid plane. 0 <= o < nbgrains: n_grain = n_grain + 1 and Sgux = Sgux + ux, Sguy = Sguy + uy if selected. Anything else (the
 * lattice-edge walls): nothing. A plane outside the node's class is left untouched (the same bits as adding +0.0: a chain from
 * +0.0 never holds -0.0). A value that is not finite is accumulated as it comes. Then samples = samples + 1.
 * Derived fields, planes [lx][ly] of doubles in ascending bit order of the field mask, count = (bits set) * lx * ly, with
 * N = (double)samples, nf = (double)n_fluid[x][y], ng = (double)n_grain[x][y]:
 *   LBMDEM_MEANF_PHI   phi   = nf / N                      LBMDEM_MEANF_SOLID solid = ng / N
 *   LBMDEM_MEANF_UX    mux   = Sux / nf                    LBMDEM_MEANF_UY    muy   = Suy / nf
 *   LBMDEM_MEANF_RXX   rxx   = (Sxx / nf) - (mux * mux)    LBMDEM_MEANF_RXY   rxy   = (Sxy / nf) - (mux * muy)
 *   LBMDEM_MEANF_RYY   ryy   = (Syy / nf) - (muy * muy)
 *   LBMDEM_MEANF_RHO   mrho  = Srho / nf                   LBMDEM_MEANF_VRHO  vrho  = (Srho2 / nf) - (mrho * mrho)
 *   LBMDEM_MEANF_DISS  mdiss = Sdiss / nf                  LBMDEM_MEANF_GDOT  mgdot = Sgdot / nf
 *   LBMDEM_MEANF_GUX   gux   = Sgux / ng                   LBMDEM_MEANF_GUY   guy   = Sguy / ng
 * and +0.0 wherever the divisor count is 0. (rxx, ryy, vrho are differences of rounded numbers: they may come out a few ulp of the
 * mean square below zero.) To SI units as in the flow-fields block; mean pore pressure P = (1. / 3.) * rho_moy * (mrho - 1.) * c^2.
 * Profile: out[14][ly]; row k < 13 is, for every y, the chain from +0.0 over x ascending of derived field k (bit k above), row 13
 * that of nf. A field whose accumulators the window does not hold gives a row of +0.0. The division by lx is left to the caller.
 *   lbmdem_mean_begin           opens a window with the planes of `mask`. An open window is discarded; its memory is kept when
 *                               the mask is the same and given back and allocated anew when it differs. The memory -- 8 bytes
 *                               of counts and 8 per selected plane for every node of the padded lattice -- comes from the
 *                               handle's pool. every >= 1: the k-th fluid step after this call, k = 1, 2, ..., is sampled when
 *                               k % every == 0, on the handle's stream behind the force kernels, the probe sample, the tracer
 *                               advance and the scalar step (lbmdem_forces_fluid; so in lbmdem_lbm_step, lbmdem_run,
 *                               lbmdem_run_scene), from the map that step took. every == 0: samples by hand only.
 *   lbmdem_mean_sample          one sample of the present state (f = lbmdem_download_f, obst = lbmdem_download_obst, the present
 *                               kinematics and walls: what lbmdem_tracer_advance reads), on the handle's stream; does not
 *                               synchronise.
 *   lbmdem_mean_reset           zeroes the window: accumulators, counts, samples. The mask, `every` and the count of hooked fluid
 *                               steps modulo `every` stay, so the cadence goes on as if nothing had happened.
 *   lbmdem_mean_end             closes the window and gives the memory back. Nothing to do without one.
 *   lbmdem_mean_stats           out5 = { 1 if a window is open else 0, its mask, samples, hook_steps: the fluid steps the hook has
 *                               counted since lbmdem_mean_begin (after a reset: modulo every), bytes the window holds }.
 *   lbmdem_mean_download        the raw accumulators: the selected planes as [lx][ly] in the order of the table above
 *                               (*count = planes * lx * ly doubles, always set; a buffer of fewer is refused), n_fluid and n_grain
 *                               as [lx][ly]. Settles and synchronises.
 *   lbmdem_mean_fields          copies the derived planes of `fmask` to the host; *count, cap_doubles as lbmdem_flow_fields.
 *                               A field whose accumulators are not in the window's mask is refused by name; a window without a
 *                               sample is refused ("no sample has been taken"). Synchronises.
 *   lbmdem_mean_fields_device   the same planes into the caller's DEVICE memory on the handle's stream; does not synchronise.
 *   lbmdem_mean_profile         out[14][ly] (cap_doubles >= 14 * ly). Synchronises.
 *   lbmdem_write_mean_files     host only, no handle, no device: <dir>/mean%.6i.vtk -- the binary rectilinear-mesh format of
 *                               flow%.6i.vtk (same header, mesh and CELL_DATA / POINT_DATA lines, big-endian float, x fastest),
 *                               "VECTORS mean_fluid_velocity_lb float\n" with (float)mux, (float)muy, 0 per node, then
 *                               "SCALARS <name> float\nLOOKUP_TABLE default\n" with the payload for fluid_fraction (phi),
 *                               fluctuation_energy (0.5 * (rxx + ryy)), reynolds_xy (rxy) and mean_density (mrho) -- and
 *                               <dir>/mean_profile%.6i.dat: the line
 *                               "# y samples phi solid mux muy rxx rxy ryy mrho vrho mdiss mgdot gux guy\n", then per y "%d %ld"
 *                               of y and samples and thirteen " %le" of p / (double)lx for the profile's rows 0..12, "\n".
 *                               Planes [lx][ly], profile14 = [14][ly]. lx, ly >= 2.
 *   lbmdem_write_mean           the same two files of the handle's window (the planes downloaded, the image made on the host);
 *                               a plane the window cannot give is +0.0, as its row of the profile is. Synchronises.
 *   lbmdem_set_mean_output      mask != 0 (every >= 1): lbmdem_run_scene (comm == NULL) with the fluid and a directory opens a
 *                               window (mask, every) at its start and, at every VTK event, after the frame and the other exports'
 *                               files, provided samples > 0, calls lbmdem_write_mean with the event's nFile and resets the
 *                               window: each file holds the averages since the event before. Synchronous. mask == 0: off (the
 *                               default).
 * Give-up recovery: a sample queued behind a launch of the multi-sub-step DEM kernel that gave up finds the stop word and adds
 * nothing; the replay repeats those fluid steps and samples again, once each; samples and hook_steps follow.
 * A sample only reads the step's state and writes the window: no call changes anything a later step reads. With no window open a
 * fluid step pays one comparison on the host; nothing is allocated or launched. A checkpoint does not carry a window or the
 * output setting: a loaded handle has none, and the file is byte for byte what a handle without one saves -- unless
 * lbmdem_set_checkpoint_contents has LBMDEM_CKPT_MEAN on: then the window's mask, `every`, accumulators and counts are in the file
 * and come back with it, hook_steps included, so that the k-th-step rule goes on in phase (never the output setting).
 * LBMDEM_EINVAL: a strip of a decomposition or distributed grains (and lbmdem_dist_enable with a window open or the output on);
 * the single-precision library (lbmdem_write_mean_files works there too); a mask of 0 or with bits beyond LBMDEM_MEAN_ALL /
 * LBMDEM_MEANF_ALL; every < 0; null arguments; a short buffer; a sample, a reset or a read without a window; a directory that
 * cannot be written ("cannot open"). Vibrating, probing, lid, tracer and scalar handles have the feature. Not built: windows on
 * strips, averages of vorticity or of the dye, weighted or several simultaneous windows, a device image kernel. */
#define LBMDEM_MEAN_U 1
#define LBMDEM_MEAN_UU 2
#define LBMDEM_MEAN_RHO 4
#define LBMDEM_MEAN_DISS 8
#define LBMDEM_MEAN_GRAIN 16
#define LBMDEM_MEAN_ALL 31
#define LBMDEM_MEANF_PHI 1
#define LBMDEM_MEANF_SOLID 2
#define LBMDEM_MEANF_UX 4
#define LBMDEM_MEANF_UY 8
#define LBMDEM_MEANF_RXX 16
#define LBMDEM_MEANF_RXY 32
#define LBMDEM_MEANF_RYY 64
#define LBMDEM_MEANF_RHO 128
#define LBMDEM_MEANF_VRHO 256
#define LBMDEM_MEANF_DISS 512
#define LBMDEM_MEANF_GDOT 1024
#define LBMDEM_MEANF_GUX 2048
#define LBMDEM_MEANF_GUY 4096
#define LBMDEM_MEANF_ALL 8191
int lbmdem_mean_begin(lbmdem_handle* h, int mask, int every);
int lbmdem_mean_sample(lbmdem_handle* h);
int lbmdem_mean_reset(lbmdem_handle* h);
int lbmdem_mean_end(lbmdem_handle* h);
int lbmdem_mean_stats(lbmdem_handle* h, long* out5);
int lbmdem_mean_download(lbmdem_handle* h, double* planes, unsigned* n_fluid, unsigned* n_grain, long cap_doubles, long* count);
int lbmdem_mean_fields(lbmdem_handle* h, int fmask, double* out, long cap_doubles, long* count);
int lbmdem_mean_fields_device(lbmdem_handle* h, int fmask, void* dev_out, long cap_doubles);
int lbmdem_mean_profile(lbmdem_handle* h, double* out, long cap_doubles);
int lbmdem_write_mean(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_write_mean_files(const char* dir, int nfile, int lx, int ly, long samples, const double* phi, const double* mux,
                            const double* muy, const double* rxx, const double* rxy, const double* ryy, const double* mrho,
                            const double* profile14);   /* host only */
int lbmdem_set_mean_output(lbmdem_handle* h, int mask, int every);   /* mask 0: off (default) */
/* write_densities (main.c:482-566), the reference's ASCII, ParaView-readable dump of the fluid fields masked by the obstacle
 * map: <dir>/densities%.6i.vtk -- the reference's header ("Outfile domain LB t: %e" with the handle's clock, coordinates
 * (float)i * (1./lx) printed "%e " on both axes), a SCALARS Pressure section of "%.4lf\n" lines and a VECTORS VecVelocity
 * section of "%.4lf %.4lf 0.\n" lines, both in file order [y][x] -- and <dir>/pressure_base%.6i.dat, "%le %le\n" per x for
 * row y == 2 (no lines when ly <= 2). Per node P = (1./3.) * rho_moy * (sum_i f[i] - 1.), u_x = sum_i f[i] * ex[i],
 * u_y = sum_i f[i] * ey[i], i = 0..8 in that order; all three +0.0 where obst >= 0. The map is the one
 * lbmdem_download_obst and lbmdem_download_vtk_fields show: what the last fluid step saw, not a rasterisation a run has
 * already made for the coming one.
 * The "%.4lf" text is made ON THE DEVICE, byte for byte what printf prints (the exact binary value rounded to nearest, ties to
 * even; "-0.0000" for -0.0 and for negatives that round to zero): a count pass, a scan and an emit pass over BANDS of whole
 * file rows, each band through a device staging buffer and pinned host memory to the file. Both buffers are bounded by the
 * staging budget -- 64 MiB unless lbmdem_set_densities_staging says otherwise (0 restores the default); a budget below the
 * file's longest row counts as that row. A section's bands hold as many rows as the budget has room for that section's
 * longest row. The device formats finite values below 1e9 in magnitude; if a single node holds anything else, the whole
 * file is written by lbmdem_write_densities_host from a download instead.
 *   lbmdem_write_densities          both files; synchronises; f, obst, the grains and every counter are left as they were
 *   lbmdem_download_densities_text  the body without the header lines: all Pressure lines, then all velocity lines. A cap that
 *                                   is too small (0 included; out may then be NULL): LBMDEM_EINVAL, *bytes = what is needed
 *   lbmdem_densities_stats          counts4, of the last of those two calls: bytes of the Pressure lines, bytes of the
 *                                   velocity lines, bands (both sections together; 0 when the host wrote the text), nodes the
 *                                   device refused to format
 *   lbmdem_write_densities_host     host only, no handle, no device: the reference's loops, one fprintf per value, over
 *                                   f[lx][ly][9] and obst[lx][ly]. Unlike the reference it checks fopen.
 *   lbmdem_format_fixed4            host only: the device's formatter on the host, every value followed by "\n"; *bytes = the
 *                                   length; LBMDEM_EINVAL for a value that is not finite or not below 1e9, or a cap too small
 * LBMDEM_EINVAL: a strip of a decomposition or distributed grains; the single-precision library (the two host-only calls
 * exist there too); null arguments; a directory that cannot be written ("cannot open"). */
int lbmdem_write_densities(lbmdem_handle* h, const char* dir, int nfile);
int lbmdem_download_densities_text(lbmdem_handle* h, char* out, size_t cap, size_t* bytes);
int lbmdem_set_densities_staging(lbmdem_handle* h, size_t bytes);
int lbmdem_densities_stats(lbmdem_handle* h, long* counts4);
int lbmdem_write_densities_host(const char* dir, int nfile, int lx, int ly, double t, double rho_moy, const double* f_aos,
                                const int* obst);
int lbmdem_format_fixed4(const double* v, long n, char* out, long cap, long* bytes);
/* The same two events written in the background while the run goes on, by the writer thread of lbmdem_set_async_output (one
 * thread and one copy stream per handle, made for whichever of the two features is switched on first; its jobs are strictly
 * first in, first out, so the lines of stats.data land in call order). lbmdem_set_async_dem(h, slots), slots in
 * 1..LBMDEM_ASYNC_MAX_DEM, sets up that many table slots (device staging + pinned host memory of LBMDEM_DEM_ROW_DOUBLES
 * doubles per grain each); 0 writes what is queued and frees them (the default: nothing is allocated, no thread exists, and
 * lbmdem_write_dem, lbmdem_write_forces and lbmdem_run_scene do what they did). A row is what DEM%06d.dat prints after the
 * index -- r x1 x2 x3 v1 v2 v3 a1 a2 a3 fhf1 fhf2 fhf3 p s ESE fr ifr ice slip rw fm M11 M12 M21 M22 z -- and zz, all as
 * doubles. lbmdem_write_dem_async settles the handle like every writer, takes a free slot -- when none is free it waits for
 * the writer: an event is never dropped --, launches two kernels on the handle's stream (the rows into the slot as the file
 * holds them; the 22 numbers of the stats.data line, whose ten sums are added in grain order by one lane each, as the host
 * loop adds them: bit-equal to lbmdem_write_dem's), queues the copy of the rows on the copy stream behind an event, waits
 * for the 22 numbers -- the only wait on the step stream --, hands the slot to the writer and returns energies8 exactly as
 * lbmdem_write_dem does. The writer formats DEM%06d.dat, appends the line to stats.data and, when with_forces, searches the
 * pairs and prints DEM%06d.ps: the files of lbmdem_write_dem + lbmdem_write_forces byte for byte. What is stepped afterwards
 * does not reach them. Failures of the writer travel as for frames: the first one is returned by the next
 * lbmdem_write_dem_async or lbmdem_write_vtk_async (which then queues nothing), lbmdem_output_drain or lbmdem_run_scene and
 * is then forgotten. lbmdem_output_drain and lbmdem_destroy cover tables as well. On a handle with tables in the background,
 * lbmdem_run_scene (comm = NULL) hands its DEM events to lbmdem_write_dem_async (with_forces = 1) and drains before it
 * returns.
 * lbmdem_dem_stats: the stats.data line of the last table sub-step alone (the two kernels without the rows, 176 bytes
 * back), feature on or off; energies8 = stats22[{8, 15, 16, 18, 17, 19, 20, 21}].
 * lbmdem_output_stats_dem -- counts4: events queued, written, failed, calls that had to wait for a slot; ms4: the caller
 * waiting for a slot, the writer waiting for copies, the writer in file I/O, the caller waiting for the 22 numbers.
 * lbmdem_write_dem_rows: host only, no handle, no device -- DEM%06d.dat, one line appended to stats.data, and DEM%06d.ps
 * (bounding box from lx, ly) when with_forces, from n rows and a stats line: the formatter and the pair search that the
 * synchronous writers and the writer thread share.
 * LBMDEM_EINVAL: slots outside 0..4, lbmdem_write_dem_async while off or without a valid table, a strip of a decomposition or
 * distributed grains (and lbmdem_dist_enable on a handle with tables in the background), the single-precision library (it
 * has no write_DEM). LBMDEM_ENOMEM: the slots cannot be had (then the feature is off). Vibrating and probing handles have it.
 * Checkpoints do not carry the setting. */
#define LBMDEM_DEM_ROW_DOUBLES 28
#define LBMDEM_ASYNC_MAX_DEM 4
int lbmdem_dem_stats(lbmdem_handle* h, double* stats22);
int lbmdem_set_async_dem(lbmdem_handle* h, int slots);            /* 0: off (default) */
int lbmdem_write_dem_async(lbmdem_handle* h, const char* dir, int nfile, int with_forces, double* energies8);
int lbmdem_output_stats_dem(lbmdem_handle* h, long* counts4, double* ms4);
int lbmdem_write_dem_rows(const char* dir, int nfile, int n, const double* rows, const double* stats22,
                          int with_forces, int lx, int ly);
/* Checkpoint / restart (absent in the reference, which cannot resume a run: SURVEY.md section 5). The file
 * holds exactly the state that defines the continuation at a renderScene() boundary -- populations,
 * current obstacle map, grain kinematics, hydrodynamic forces, Verlet lists, wall positions, step
 * counter, the force-kernel choice, the diagnostics switch and the "previous contact" carries of the
 * order-dependent diagnostics -- in the device layout of the strip that wrote it (a layout word in the
 * header rejects files of another layout). A run restarted from it is bit-identical to the uninterrupted
 * run. load creates a new handle on `device`. */
int lbmdem_checkpoint_save(lbmdem_handle* h, const char* path);
int lbmdem_checkpoint_load(const char* path, int device, lbmdem_handle** out);
/* Checkpoints on a cadence, written in the background, replaced atomically, with digests. lbmdem_set_async_checkpoint(h,
 * slots), slots in 1..LBMDEM_ASYNC_MAX_CKPT, sets up that many checkpoint slots (device staging + pinned host memory of the
 * file's size, the pair list at its capacity) on the copy stream, writer thread and queue of lbmdem_set_async_output; 0
 * switches it off again (writes what is queued first); off is the default, and then nothing is allocated.
 * lbmdem_checkpoint_save_async settles the handle like lbmdem_checkpoint_save, takes a free slot -- when none is free it waits
 * for the writer, a checkpoint is never dropped --, notes the host's side of the header as it stands, gathers every
 * device-resident section into the slot with ONE kernel on the handle's stream (which also adds up the sections' digests and
 * reads the pair list's length and the carries on the device), queues the copy to host memory behind it on the copy stream
 * and returns without synchronising: nothing stepped afterwards reaches the file. The writer thread writes `<path>.tmp`,
 * closes it and renames it onto `<path>`: at every instant `<path>` is the previous complete checkpoint or the new one; on
 * failure the .tmp file is removed and `<path>` is not touched. The failure is handed over like a frame's or a table's: returned
 * once by the next lbmdem_*_async call (which then queues nothing), lbmdem_output_drain or lbmdem_run_scene.
 * The file is lbmdem_checkpoint_save's, byte for byte, followed by a digest trailer: "LBMCKSM1", int nsections (10), int 0,
 * then per section {uint64 bytes, uint64 S1, uint64 S2} in file order -- header, r, kin, fhf, gp, offsets, nbr, wallflags,
 * obst, f. Of a section's little-endian 64-bit words w_0 .. w_{W-1} (the last zero-padded) S1 = sum w_i and S2 = sum (i + 1)
 * w_i, both mod 2^64: lbmdem_checkpoint_digest (host only). lbmdem_checkpoint_verify (host only, no device) recomputes every
 * section of a file against its trailer: LBMDEM_EINVAL naming the first section that differs, or for a trailer that is cut
 * short; LBMDEM_OK with *has_digest = 0 for a file without a trailer (lbmdem_checkpoint_save's). lbmdem_checkpoint_load verifies a
 * file that has a trailer first and refuses it when it does not match; a file without one loads as before.
 * lbmdem_set_checkpoint_every(h, every_substeps, path): on such a handle lbmdem_run_scene (comm = NULL) ends a stretch at
 * every step counter that is a multiple of every_substeps and saves to `path` there, after that sub-step's other events --
 * through lbmdem_checkpoint_save_async when slots exist, else with lbmdem_checkpoint_save by way of `<path>.tmp` and rename -- and
 * drains before it returns. Its schedule, console lines and other files are unchanged. 0 is off (the default).
 * lbmdem_output_stats_checkpoint: as lbmdem_output_stats; ms4[3] is the time callers spent in lbmdem_checkpoint_save_async
 * behind their slot. LBMDEM_EINVAL: slots outside 0..2, lbmdem_checkpoint_save_async while off, a strip of a decomposition or
 * distributed grains (and lbmdem_dist_enable on a handle that has either setting on), the single-precision library (it has no
 * checkpoints). LBMDEM_ENOMEM: the slots cannot be had (then the feature is off). Vibrating and probing handles have it. A
 * checkpoint carries neither setting.
 *
 * The optional state. lbmdem_set_checkpoint_contents(h, mask), mask an OR of LBMDEM_CKPT_TRACERS, LBMDEM_CKPT_SCALAR,
 * LBMDEM_CKPT_MEAN (0: off, the default), makes every save of the handle -- lbmdem_checkpoint_save, lbmdem_checkpoint_save_async,
 * the cadence of lbmdem_run_scene -- add what of the three the handle has at that moment: the tracers (positions, `automatic`,
 * both counts), the passive scalar (populations, the fluid flags `was`, tau_s, `automatic`, both counts; omega is formed from
 * tau_s again, scratch buffers are not stored) and the open averaging window (mask, `every`, n_fluid, n_grain, the selected
 * planes, samples and hook_steps). lbmdem_checkpoint_load needs no setting: it restores whatever the file holds, through the same
 * allocations as lbmdem_tracer_set, lbmdem_scalar_set and lbmdem_mean_begin, and a run continued from the file is bit-identical
 * in all three to the uninterrupted one. With the mask 0, or with nothing of the mask present on the handle, the file is the
 * plain file byte for byte and its trailer "LBMCKSM1". The setting is not stored in the file, nor are the per-frame output
 * settings or the probes' ring. lbmdem_run_scene, which opens a new window on entry (lbmdem_set_mean_output), goes on with a
 * window that has just been loaded instead -- once -- when its mask and `every` are those of the output setting.
 * Layout. Behind section f, and only in a file of a whole handle (has_dist == 0), the extension: a header of 120 bytes, little
 * endian -- "LBMXTRA1"; int32 mask, int32 0; int64 lx * sy (a sanity value; sy: the row pitch, ly rounded up to 16);
 * tracers: int64 n, int32 automatic, int32 0, int64 advances, int64 hook_advances; scalar: float64 tau_s, int32 automatic,
 * int32 0, int64 steps, int64 hook_steps; window: int32 mask, int32 every, int32 nsel (planes of doubles), int32 0, int64
 * samples, int64 hook_steps; the values of a state the mask does not name are 0 -- then five sections in this order, each of
 * length 0 when its bit is clear: tracers (16 n bytes: x, y per tracer), scalar_g (five planes of lx * sy doubles, device
 * layout [x][sy]), scalar_was (lx * sy bytes, each 0 or 1), mean_cnt (two planes of lx * sy uint32), mean_S (nsel planes of lx *
 * sy doubles). A background file with an extension ends in the trailer "LBMCKSM2" instead of "LBMCKSM1": the same form with
 * always 16 entries -- the ten above, then extras (the extension header), tracers, scalar_g, scalar_was, mean_cnt, mean_S; an
 * absent section has bytes, S1 and S2 of 0 --, so either trailer is found at the very end of a file. lbmdem_checkpoint_verify
 * and the loader accept both and name the section that fails. The loader trusts nothing of the extension: lengths against the
 * file's size, n within the tracers' limit and every position inside the lattice (NaN refused), tau_s finite and > 0.5, `was`
 * bytes 0 or 1, the window's mask, nsel and counters; a file whose extension fails is refused as a whole. A library from before
 * the extension loads such a file as a plain one: it stops reading behind f (and does not see the trailer "LBMCKSM2" of a
 * background file, whose digests it therefore does not check).
 * lbmdem_checkpoint_contents(path, out5) (host only, no device): what a file carries -- out5 = {mask, tracers, the scalar's
 * steps, the window's mask, the window's samples}; all 0 for a plain file.
 * LBMDEM_EINVAL: bits beyond LBMDEM_CKPT_ALL; a non-zero mask on a strip of a decomposition or with distributed grains; the
 * single-precision library. lbmdem_checkpoint_save_async makes its slots larger (as many, after draining them) when the state has
 * outgrown them; LBMDEM_ENOMEM from that leaves checkpoints in the background off. */
#define LBMDEM_CKPT_TRACERS 1
#define LBMDEM_CKPT_SCALAR 2
#define LBMDEM_CKPT_MEAN 4
#define LBMDEM_CKPT_ALL 7
int lbmdem_set_checkpoint_contents(lbmdem_handle* h, int mask);   /* 0: off (default) */
int lbmdem_checkpoint_contents(const char* path, long* out5);
#define LBMDEM_ASYNC_MAX_CKPT 2
int lbmdem_set_async_checkpoint(lbmdem_handle* h, int slots);     /* 0: off (default) */
int lbmdem_checkpoint_save_async(lbmdem_handle* h, const char* path);
int lbmdem_output_stats_checkpoint(lbmdem_handle* h, long* counts4, double* ms4);
int lbmdem_set_checkpoint_every(lbmdem_handle* h, long every_substeps, const char* path);   /* 0: off (default) */
int lbmdem_checkpoint_digest(const void* bytes, size_t n, unsigned long long* out2);      /* S1, S2 */
int lbmdem_checkpoint_verify(const char* path, int* has_digest);
long lbmdem_nbsteps(lbmdem_handle* h);
/* (drains the stream when launches of the multi-sub-step kernel are unconfirmed: the sub-steps asked for before this call
 * are counted from the old value, the ones after it from n) */
int lbmdem_set_nbsteps(lbmdem_handle* h, long n);
int lbmdem_get_config(lbmdem_handle* h, lbmdem_config* out);

/* ---- streams, timing, multi-GPU plumbing ------------------------------------------------------ */

/* Enqueue on a caller-owned hipStream_t (NULL is the HIP default stream -- what PyTorch calls its
 * default stream), e.g. so that work is ordered with torch.distributed collectives; the library's
 * private non-blocking stream is the default and lbmdem_use_own_stream() goes back to it. */
int lbmdem_set_stream(lbmdem_handle* h, void* hip_stream);
int lbmdem_use_own_stream(lbmdem_handle* h);
int lbmdem_sync(lbmdem_handle* h);
/* HIP-event timing of the dominant kernel (fused collide+stream), on the stream it is launched on.
 * enable, run steps, then read the mean duration and the launch count. on = N > 1: every N-th launch is timed (the two
 * event records around a launch hold the next dispatch back: ~10 us per coupled step when every launch is timed). */
int lbmdem_profile_enable(lbmdem_handle* h, int on);
int lbmdem_profile_read(lbmdem_handle* h, double* mean_ms, long* launches);
/* GB/s (bytes read + bytes written) of a plain copy kernel moving `bytes` on this handle's device and stream: the best of
 * four shapes (8 or 16 bytes per lane, 2 048 to 8 192 workgroups), each the best of `reps` passes after a warm-up: the
 * yardstick bench.py puts next to the fused kernel's traffic rate (boxes differ by +-5 %). */
int lbmdem_measure_copy(lbmdem_handle* h, size_t bytes, int reps, double* gb_per_s);

/* Strip decomposition along x (one process per GPU); halo >= 2 rows (with REPLICATED grains, i.e. without
 * lbmdem_dist_enable, halo >= 2 + the largest grain radius in nodes). After collide_stream the `halo` outermost
 * OWNED rows on each interior side are packed into a caller-provided DEVICE buffer
 * (9 * halo * ly doubles, plane-major), exchanged by the caller (RCCL send/recv via
 * torch.distributed) and unpacked into the neighbour's halo rows. side: 0 = low x, 1 = high x. */
long lbmdem_halo_doubles(lbmdem_handle* h);
/* collide_stream in two parts, so that the halo exchange overlaps the bulk of the kernel:
 *   LBMDEM_CS_EDGES     the owned rows within `halo` of an interior cut (what the neighbours need); the
 *                       new lattice becomes current, halo_pack may follow immediately;
 *   LBMDEM_CS_INTERIOR  the remaining owned rows. Must follow EDGES before anything else reads the
 *                       lattice (forces_fluid, downloads, the next collide_stream fail until then).
 * EDGES + INTERIOR == lbmdem_collide_stream, row for row (every row is computed from the old lattice). */
#define LBMDEM_CS_EDGES 1
#define LBMDEM_CS_INTERIOR 2
int lbmdem_collide_stream_part(lbmdem_handle* h, int part);
int lbmdem_halo_pack(lbmdem_handle* h, int side, void* dev_buf);
int lbmdem_halo_unpack(lbmdem_handle* h, int side, const void* dev_buf);
int lbmdem_halo_pack2(lbmdem_handle* h, void* buf_lo, void* buf_hi);   /* both sides in one launch; null skips a side */
int lbmdem_halo_unpack2(lbmdem_handle* h, const void* buf_lo, const void* buf_hi);
/* ---- strips with the GRAINS distributed over the ranks (no collective) ------------------------------------------
 * Every rank keeps arrays for all grains (global index = array index) but integrates only the grains whose centre
 * lies in its rows plus a margin of `margin_rows` on either side, deep enough that what it does not integrate cannot
 * influence an owned grain within the npDEM sub-steps between two fluid steps (one Verlet-list edge per sub-step).
 * Per fluid step, with both neighbours, three point-to-point messages (fixed capacities, device buffers):
 *   LBMDEM_MSG_KIN     kinematics of the owned grains within the neighbour's margin -- also how a grain that crossed
 *                      the cut changes owner; may travel while the fluid step runs, unpack before the sub-steps;
 *   LBMDEM_MSG_TABLES  this rank's part of the link-sum tables of grains the neighbour owns (packed after
 *                      collide_stream and the f halo exchange, unpacked by the owner before forces_fluid);
 *   LBMDEM_MSG_FHF     hydrodynamic forces of the grains of the KIN message (after forces_fluid, before the sub-steps).
 * Sequence of one period: dist_begin_period; pack KIN (both sides); obst_construction; collide_stream (or its two
 * parts + halo exchange); pack TABLES / exchange / unpack TABLES; forces_fluid; unpack KIN; pack FHF / exchange /
 * unpack FHF; run_dem(npDEM). Results equal the single-GPU run bit for bit for any number of strips.
 * Needs halo >= 2 only. Overlapping reduced discs across a cut, or more grains near a cut than the message
 * capacities, are reported by lbmdem_sync. write_DEM's order-dependent diagnostics are not available in this mode. */
#define LBMDEM_MSG_KIN 0
#define LBMDEM_MSG_FHF 1
#define LBMDEM_MSG_TABLES 2
int lbmdem_dist_default_margin(lbmdem_handle* h);          /* rows */
int lbmdem_dist_margin_for(const lbmdem_config* cfg, double rmax_m);   /* the same from a derived config and the largest radius (host only) */
int lbmdem_dist_enable(lbmdem_handle* h, int margin_rows); /* 0 = default; the strip must be at least that wide */
long lbmdem_dist_message_doubles(lbmdem_handle* h, int kind); /* capacity of one message, in doubles */
int lbmdem_dist_begin_period(lbmdem_handle* h);
int lbmdem_dist_pack(lbmdem_handle* h, int kind, int side, void* dev_buf);
int lbmdem_dist_unpack(lbmdem_handle* h, int kind, int side, const void* dev_buf);
/* both sides in one launch (a null buffer skips the side): fewer dependent kernel launches per fluid step */
int lbmdem_dist_pack2(lbmdem_handle* h, int kind, void* buf_lo, void* buf_hi);
int lbmdem_dist_unpack2(lbmdem_handle* h, int kind, const void* buf_lo, const void* buf_hi);

/* ---- RCCL transport of that protocol for a C host (the driver 2d-lbm-dem_amd/host/lbmdem --gpus N); strips.py does
 * the same over torch.distributed. One process per GPU; rank k talks to ranks k-1 and k+1 only: ncclSend / ncclRecv
 * grouped per message class on side streams (the kinematics and the f halo rows travel while kernels run), no
 * collective on the step path. RCCL is dlopen'ed by the first of these calls. */
#define LBMDEM_COMM_ID_BYTES 512          /* four RCCL unique ids: one communicator per message class */
int lbmdem_comm_unique_id(void* id);      /* rank 0 makes it, every rank passes the same bytes to ..._create */
int lbmdem_comm_create(const void* id, int rank, int world, int device, lbmdem_comm** out);
int lbmdem_comm_destroy(lbmdem_comm* c);
/* one fluid step of a handle in distributed-grain mode with its neighbours (the sequence documented above) */
int lbmdem_comm_lbm_step(lbmdem_handle* h, lbmdem_comm* c);
/* n x renderScene() (main.c:1697-1765) with that fluid step */
int lbmdem_comm_run(lbmdem_handle* h, lbmdem_comm* c, long n_dem_steps);
/* Drop-in outputs of a strip decomposition (not on the step path; output cadence).
 * The sub-step that feeds write_DEM -- the one that brings the step counter to a multiple of 4000, main.c:1773 -- is
 * run by ONE rank on a full replica, because four columns of the table (fr, ice, slip, rw) thread "previous contact"
 * carries through all contacts in grain-index order (main.c:130-131):
 *   lbmdem_dist_export_owned   state12 [n][12] (9 kinematic columns + fhf1..3) of the grains this rank owns, zeros
 *                              elsewhere; owned [n]; per carry the youngest record among the owned grains' contacts:
 *                              carry_keys [3][2] ({0,0} = none since the last table sub-step), carry_vals [3]
 *   (the caller merges the exports: disjoint, every grain has one owner; per carry the greatest key pair wins)
 *   lbmdem_dist_table_substep  the root imports the merged state, rebuilds its Verlet list from it and runs the
 *                              sub-step for all n grains with the single-domain diagnostic pipeline; afterwards
 *                              lbmdem_download_grain_table / lbmdem_write_dem / lbmdem_write_forces work on it.
 * lbmdem_comm_run does all of this over RCCL (rank 0 = root). write_vtk: lbmdem_vtk_place_owned drops the owned
 * columns into zeroed lattice-sized arrays (fields11: grain_pressure[cnt], grain_velocity[3 cnt],
 * grain_acceleration[3 cnt], fluid_pressure[cnt], fluid_velocity[3 cnt], each [ly][lx]), the merged arrays go to
 * lbmdem_write_vtk_fields; lbmdem_comm_write_vtk = both over RCCL, rank 0 writes. */
int lbmdem_dist_export_owned(lbmdem_handle* h, double* state12, unsigned char* owned, long long* carry_keys,
                             double* carry_vals);
int lbmdem_dist_table_substep(lbmdem_handle* h, const double* state12_full, const double* carry_vals,
                              const int* carry_has);
int lbmdem_vtk_place_owned(lbmdem_handle* h, float* fields11);
int lbmdem_write_vtk_fields(const char* dir, int nfile, int lx, int ly, const float* fields11);
int lbmdem_comm_write_vtk(lbmdem_handle* h, lbmdem_comm* c, const char* dir, int nfile);
/* Checkpoints of a strip decomposition: every rank saves its own handle (lbmdem_checkpoint_save: its strip, the grains
 * as it holds them, ownership masks, message capacities) and lbmdem_checkpoint_load brings it back with the grains
 * distributed again. The "previous contact" carries are agreed over the ranks first: lbmdem_dist_export_carries gives
 * a rank's youngest records and its standing values, lbmdem_dist_set_carries installs the result (per carry the
 * greatest key pair over all ranks, else rank 0's standing value); lbmdem_comm_sync_carries = both over RCCL. */
int lbmdem_dist_export_carries(lbmdem_handle* h, long long* carry_keys, double* carry_vals, double* carry_standing);
int lbmdem_dist_set_carries(lbmdem_handle* h, const double* carry3);
int lbmdem_comm_sync_carries(lbmdem_handle* h, lbmdem_comm* c);
/* bitwise merge (integer sum) of host buffers whose non-zero bits are disjoint across the ranks; in place */
int lbmdem_comm_allreduce_bits(lbmdem_comm* c, void* host_buf, size_t nbytes);
/* sum of host values over the ranks (check_density / final_density; not on the step path) */
int lbmdem_comm_allreduce_sum(lbmdem_comm* c, double* values, int n);
/* a grouped send + receive of `doubles` values from this rank to itself on a side stream while another stream is
 * busy (the transport exercised on a one-GPU box); with several ranks also the step's own pattern: on every lane one
 * grouped exchange with both neighbours, all lanes in flight at once, payload checked. Collective over the ranks. */
int lbmdem_comm_selftest(lbmdem_comm* c, int doubles);

/* Device pointer to the 3*n hydrodynamic-force table (fhf1[n], fhf2[n], fhf3[n]) and to the
 * n-entry ownership mask (1 = this rank computed the grain) for the cross-rank combine. */
int lbmdem_fhf_device(lbmdem_handle* h, void** fhf, void** owner_mask);
/* Cross-rank combine of the hydrodynamic forces: forces_fluid writes the forces of the grains this
 * rank owns and exact zeros for the others, so a bit-wise integer SUM all-reduce of the exported
 * table (3*n doubles viewed as int64) reconstructs every grain's force exactly. export/import copy
 * the table to/from a caller-provided DEVICE buffer on the handle's stream. */
int lbmdem_fhf_export(lbmdem_handle* h, void* dev_buf);
int lbmdem_fhf_import(lbmdem_handle* h, const void* dev_buf);

const char* lbmdem_last_error(void);
const char* lbmdem_version(void);

/* ---- test aids -----------------------------------------------------------------------------------
 * Nothing a host needs; the GPU test suite checks the library's short cuts against its own slow paths through these.
 * Collected here so that the list above is the product's surface:
 *   lbmdem_set_change_mask(h, 2)   every fused launch is repeated with both maps read everywhere and compared (above)
 *   lbmdem_set_dem_chain(h, -1)    runs of sub-steps without the rasterisation at their end (above)
 *   lbmdem_set_obst_update(h, 0), lbmdem_set_dem_chain(h, 0), lbmdem_set_change_mask(h, 0), lbmdem_set_force_mode(h, 1)
 *                                  the A/B switches of bench.py (--obst-update, --dem-chain, --change-mask, --force-mode)
 *   the *_stats / lbmdem_dem_chain_paints / lbmdem_dem_chain_recoveries counters
 *   LBMDEM_RCCL_LIBRARY            (environment) the RCCL library lbmdem_comm_create loads; the tests point it at
 *                                  tests/rccl_shim to run several ranks on ONE GPU; announced on stderr when set
 * and, only here: */
/* after every sub-step, grains this rank does not integrate are overwritten with NaN (strip tests: nothing may read them) */
int lbmdem_dist_set_poison(lbmdem_handle* h, int on);

#pragma pop_macro("duration")
#pragma pop_macro("scale")
#pragma pop_macro("ly")
#pragma pop_macro("lx")

#ifdef __cplusplus
}
#endif
#endif
