/*
 * lbmdem -- host driver in C over the C ABI (include/lbmdem_hip.h), a drop-in for the reference
 * binary: `lbmdem <sample.data>` (usage check main.c:1791-1794), same console lines
 * (main.c:614,619,656,1845,1856,1259,1885-1889) and the `final_density:` line on stderr that the
 * reference's JUBE benchmark parses (main.c:1272, benchmark.xml:101).
 *
 * The reference fixes the lattice size and the run length at compile time (-Dlx -Dly,
 * `#define duration 1.5`, main.c:27-32,47); here the same defaults apply and can be overridden at
 * run time: --lx N --ly N --scale S --duration SECONDS --steps N_DEM_STEPS --device K, and (absent in
 * the reference, which cannot resume) --checkpoint FILE (written at the end) / --restart FILE.
 * --dry: the reference compiled without `#define _FLUIDE_` (main.c:16) -- DEM only: no fluid step and no check_density
 * line (main.c:1709-1719), no VTK frames although nFile still advances (main.c:1767-1772), hydrodynamic forces 0.
 * --vib [--vib-freq F --vib-amp A]: the reference's shaken box, `vib = 1` (main.c:162-165,1700-1705): the left and right
 * walls move by amp*sin(freq*t) every DEM step (defaults freq = 5, amp = 4e-4 as main.c:163-164 initialises them); also
 * with --dry. Single GPU only.
 * --run-stats: one more line on stderr at the end, `dem_chain: launches L substeps S recoveries R paints P`: how many
 * launches of the multi-sub-step DEM kernel covered how many sub-steps, how many had to be undone, how many rasterised.
 * --probes FILE [--probe-every K] [--probe-row Y] [--probe-point X,Y ...]: the device-side probes (lbmdem_probe_*): every K-th
 * fluid step (default every one) the library records the pressure profile of lattice row Y (default 2, write_densities'
 * pressure_base row, main.c:522-541), the velocity profile, the pressure at the given nodes, xgrainmax and height; the records
 * are fetched at every check_density line (where the run synchronises anyway) and at the end. FILE gets one line per record, `step time xgrainmax height` and
 * the point pressures, and every record its own pressure_base%.6i.dat in the reference's format (main.c:495,532), numbered by
 * the record. Single GPU only.
 * --async-output [N]: VTK frames are written in the background (lbmdem_set_async_output, N = 1..4 frame slots, default 2):
 * the run goes on while a frame is copied and written; same files. The frames still in flight at the end are waited for
 * before `time:` is taken. With --run-stats one more line, `async_output: queued Q written W failed F slot_waits S
 * ms_slot_wait .. ms_copy_wait .. ms_io .. ms_drain ..` (lbmdem_output_stats). Single GPU only.
 * --async-dem [N]: the write_DEM / write_forces events are written in the background as well (lbmdem_set_async_dem, N = 1..4
 * table slots, default 2): the loop waits for the 22 numbers of the stats.data line only; formatting, pair search and file
 * I/O happen on the writer thread; same files. Waited for before `time:` like the frames. With --run-stats one more line,
 * `async_dem: queued Q written W failed F slot_waits S ms_slot_wait .. ms_copy_wait .. ms_io .. ms_stats_wait ..`
 * (lbmdem_output_stats_dem). Single GPU only.
 * --checkpoint-every N (needs --checkpoint FILE): FILE is also written whenever the step counter reaches a multiple of N DEM
 * steps (lbmdem_set_checkpoint_every), always by way of FILE.tmp and rename: FILE is a complete checkpoint at every instant.
 * --async-checkpoint [N]: those checkpoints and the final one are snapshotted by one kernel and written in the background
 * (lbmdem_set_async_checkpoint, N = 1..2 slots, default 1), with a digest trailer that --restart checks. With --run-stats one more
 * line, `async_checkpoint: queued Q written W failed F slot_waits S ms_slot_wait .. ms_copy_wait .. ms_io .. ms_hold ..`
 * (lbmdem_output_stats_checkpoint). Both single GPU only. --verify-checkpoint FILE: checks FILE against its digests without a
 * GPU and exits: 0 for a file that matches or has no digests, 1 with the section that differs.
 * --dump-geometry DIR: after the run's last sub-step and before the `final_density:` line, the reference's obst_writing
 * (main.c:1601-1641) for the most recent rasterisation: DIR/obst_LB.dat, DIR/active_nodes.dat, DIR/links.dat
 * (lbmdem_write_obst). With --run-stats one more line, `geometry: solid_nodes A active_nodes B links C links_near D links_far E
 * solid_slots F` (lbmdem_geometry_stats). Single GPU only.
 * --densities DIR: at the same place, the reference's write_densities (main.c:482-566) with the run's frame counter:
 * DIR/densities%.6i.vtk and DIR/pressure_base%.6i.dat, the text made on the device (lbmdem_write_densities), and one line after
 * `final_density:`, `densities: pressure_bytes P velocity_bytes V bands B` (lbmdem_densities_stats). Single GPU only, and not
 * with --dry (there is no fluid).
 * --contacts: the contact network of every DEM event next to its table (lbmdem_set_contacts_output): contacts%.6i.dat, one line
 * per touching pair and wall contact of the table sub-step, and DEM%.6i_chains.ps, the map with every contact drawn as wide as
 * its normal force. Single GPU only.
 * --clusters [K] [--clusters-abs F] [--clusters-zmin Z]: force chains of every DEM event (lbmdem_set_clusters_output): the contacts
 * that carry at least K times the mean normal force (K defaults to 1), or at least F newtons with --clusters-abs, read as a graph --
 * clusters%.6i.dat with every grain's cluster, degree and whether it survives the removal of grains with fewer than Z contacts
 * (Z defaults to 2), cluster_table%.6i.dat, DEM%.6i_clusters.ps with the chains coloured by cluster, and a line of clusters.data.
 * Single GPU only.
 * --structure RCUT [--structure-bins N] [--structure-shell S]: the packing structure of every DEM event
 * (lbmdem_set_structure_output): the neighbours of every grain within RCUT metres, the pair histogram behind g(r) in N bins (64),
 * the bonds within S times the sum of two radii (1.2) and the bond-order and fabric sums -- structure%.6i.dat, gr%.6i.dat and a line
 * of structure.data. Single GPU only.
 * --voronoi RCUT: the Voronoi cells of every DEM event (lbmdem_set_voronoi_output): the radical tessellation of the discs inside the
 * walls from the neighbours within RCUT metres -- per grain the cell's area, perimeter, local solid fraction and topological
 * neighbour count in voronoi%.6i.dat, and a line of voronoi.data. Single GPU only.
 * --strain RCUT [--strain-incremental]: the strain fields of every DEM event (lbmdem_set_strain_output): the first event marks the
 * grains where they are, with their neighbours within RCUT metres, as the reference state; every event writes per grain the
 * displacement since the mark, the strain of its neighbourhood (a least-squares fit over the marked neighbours), D2min and the
 * neighbours lost in strain%.6i.dat, and a line of strain.data. --strain-incremental marks anew after every event: the files then
 * describe the motion between two events. Single GPU only.
 * --pores [4|8] [--pores-plane]: the pore space of every DEM event (lbmdem_set_pores_output): the fluid phase of the obstacle map
 * labelled into components joined along 4 or 8 (the default) directions -- per component its nodes, extent, walls, wetted links and
 * fluid mass in pore_table%.6i.dat, per grain the pores it borders in pore_grains%.6i.dat, a line of pores.data (is the pore space
 * one? how much fluid is trapped?) and, with --pores-plane, the label plane in pores%.6i.vtk. Single GPU only.
 * --clearance [--clearance-plane]: the pore clearance of every DEM event (lbmdem_set_clearance_output): the exact squared distance
 * from every fluid node to the nearest node that is not fluid and that node's owner -- per pair of owners whose regions meet the
 * length of the ridge and its narrowest place in throats%.6i.dat, the pore-size distribution in clearance_hist%.6i.dat, per owner
 * its fluid nodes in clearance_owners%.6i.dat, a line of clearance.data (how narrow is the narrowest throat?) and, with
 * --clearance-plane, the two planes in clearance%.6i.vtk. Single GPU only.
 * --network [MERGE] [--network-plane]: the pore network of every DEM event (lbmdem_set_network_output): the watershed of the
 * clearance map -- per pore body its peak, size and neighbours in network_bodies%.6i.dat, the groups that bodies whose pass lies
 * within MERGE of the lower summit's radius form (default: no merging) in network_groups%.6i.dat, the links between the groups
 * with their saddles in network_links%.6i.dat, a line of network.data (how many pores? how narrow is the narrowest constriction?)
 * and, with --network-plane, the body and group planes in network%.6i.vtk. Single GPU only.
 * --netflux [LEVEL] [--netflux-merge M]: the pore fluxes of every DEM event (lbmdem_set_netflux_output): the mass that crossed
 * every throat of the pore network in the last streaming step, between the bodies (LEVEL 0, the default) or the groups merged
 * within M (LEVEL 1; M default -1, no merging), in netflux_links%.6i.dat, per pore its mass, net inflow and throughput in
 * netflux_regions%.6i.dat, the net mass through every section of the lattice in netflux_profile%.6i.dat and a line of
 * netflux.data. Single GPU only.
 * --netsolve FROM --netsolve-to TO [--netsolve-band N] [--netsolve-level L] [--netsolve-merge M] [--netsolve-rtol R]
 * [--netsolve-max-iter K]: the network pressures of every DEM event (lbmdem_set_netsolve_output): the pore network as a resistor
 * network, the regions within N nodes (default 1) of the sides FROM, letters out of BTLR, at pressure 1 and those of TO at 0, a
 * link's conductance from its saddle, solved to the relative residual R (default 1e-8) in at most K iterations (default 0: the
 * number of free regions) between the pore bodies (L 0, the default) or the groups merged within M (L 1; M default -1) -- per
 * region its pressure and net inflow in netsolve_regions%.6i.dat, per link its conductance and flow in netsolve_links%.6i.dat,
 * the totals in a line of netsolve.data. Single GPU only.
 * --drainage FROM [--drainage-to TO] [--drainage-band N] [--drainage-plane]: the drainage analysis of every DEM event
 * (lbmdem_set_drainage_output): the largest disc that reaches each pore from the sides FROM, letters out of BTLR, through a
 * reservoir N nodes deep (default 1) -- the intrusion curve next to the pore-size distribution in drainage_curve%.6i.dat, per pore
 * body the size that reaches it in drainage_bodies%.6i.dat, a line of drainage.data (what passes from FROM to the sides TO, and
 * through how many candidate throats?) and, with --drainage-plane, the access plane in drainage%.6i.vtk. Single GPU only.
 * --geodesic FROM [--geodesic-to TO] [--geodesic-band N] [--geodesic-conn 4|8] [--geodesic-min-d2 D] [--geodesic-plane]: the
 * geodesic analysis of every DEM event (lbmdem_set_geodesic_output): the length of the shortest path through the fluid nodes with
 * clearance d2 >= D (default 0: all) from the sides FROM, letters out of BTLR, N nodes deep (default 1), in steps of 5 along an
 * axis and, with 8 neighbours (the default), 7 along a diagonal -- the profile over the depth behind FROM with the tortuosity in
 * geodesic_profile%.6i.dat, a line of geodesic.data (how long is the shortest way from FROM to the sides TO?) and, with
 * --geodesic-plane, the planes dist, back and detour in geodesic%.6i.vtk. Single GPU only.
 * --coarse CWxCH: the coarse-grained fields of every DEM event next to its table (lbmdem_set_coarse_output): coarse%.6i.dat, one
 * line per cell of CW x CH lattice nodes with the sums of fluid, grains and contacts over it. Single GPU only.
 * --flow: the flow fields (lbmdem_set_flow_output): flow%.6i.vtk next to every VTK frame -- composite velocity, vorticity, shear
 * rate and dissipation in lattice units -- and one line of the fluid's sums in flow.data at every DEM event. Single GPU only.
 * --tracers NXxNY: fluid tracers (lbmdem_tracer_set, lbmdem_set_tracer_output): a uniform grid of NX x NY massless particles,
 * px = (i + 0.5) * (lx - 1) / NX and py likewise, grain interiors included (those ride with their grain), advanced on the device
 * at every fluid step; tracers%.6i.vtk next to every VTK frame. Single GPU only.
 * --dye X0,Y0,X1,Y1 [--dye-tau T]: a passive scalar (lbmdem_scalar_set, lbmdem_set_scalar_output): C = 1 at the nodes X0 <= x <= X1,
 * Y0 <= y <= Y1 and 0 elsewhere, advected by the fluid and diffused on the device at every fluid step; scalar%.6i.vtk next to
 * every VTK frame and a line of scalar.data at every DEM event. T is the relaxation time, diffusivity (T - 0.5) / 3 in lattice
 * units; the default 0.53 gives 0.01, a dye that is stirred long before it spreads on its own. Single GPU only.
 * --mean [EVERY]: time-averaged flow statistics (lbmdem_set_mean_output, every accumulator): every EVERY-th fluid step (default 1)
 * is sampled on the device; mean%.6i.vtk -- mean fluid velocity, fluid fraction, fluctuation energy, Reynolds shear stress, mean
 * density -- and mean_profile%.6i.dat next to every VTK frame, each over the fluid steps since the frame before. Single GPU only.
 * --gpus N: one process per GPU, rank k on device K + k; --devices a,b,c names the device of every rank instead (the
 * same device may appear twice: that is how the tests run several ranks on a one-GPU box, see tests/rccl_shim).
 */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <math.h>
#include <unistd.h>
#include <sys/wait.h>
#include <signal.h>

#include "../../include/lbmdem_hip.h"

#define DIE(rc, what) do { if ((rc) != LBMDEM_OK) { fprintf(stderr, "%s: %s\n", what, lbmdem_last_error()); return EXIT_FAILURE; } } while (0)

/* --gpus N: one process per GPU (forked before anything touches the HIP runtime), x-strips with the grains
 * distributed, neighbour messages over RCCL (lbmdem_comm_*). Rank 0 creates the RCCL id and hands it to the others
 * through a file in a private temporary directory. Rank 0 prints and writes the VTK frames and DEM tables (merged over the ranks); checkpoints are single-GPU. */
static int g_rank = 0, g_world = 1, g_use_comm = 0, g_dry = 0, g_vib = 0, g_run_stats = 0;
static const char* g_dump_geometry = NULL;   /* --dump-geometry DIR */
static const char* g_densities = NULL;       /* --densities DIR */
static int g_contacts = 0;       /* --contacts */
static int g_flow = 0;           /* --flow */
static int g_clusters = 0, g_clusters_rel = 1, g_clusters_zmin = 2;   /* --clusters [K], --clusters-abs F, --clusters-zmin Z */
static double g_clusters_fmin = 1.;
static int g_structure = 0, g_structure_bins = 64;   /* --structure RCUT, --structure-bins N, --structure-shell S */
static double g_structure_rcut = 0., g_structure_shell = 1.2;
static int g_voronoi = 0;        /* --voronoi RCUT */
static double g_voronoi_rcut = 0.;
static int g_strain = 0;         /* --strain RCUT */
static double g_strain_rcut = 0.;
static int g_strain_incremental = 0;   /* --strain-incremental */
static int g_pores = 0, g_pores_conn = 8, g_pores_plane = 0;   /* --pores [4|8], --pores-plane */
static int g_clearance = 0, g_clearance_plane = 0;   /* --clearance, --clearance-plane */
static int g_network = 0, g_network_merge = -1, g_network_plane = 0;   /* --network [MERGE], --network-plane */
static int g_netflux = 0, g_netflux_level = 0, g_netflux_merge = -1, g_netflux_merge_set = 0;   /* --netflux [LEVEL], --netflux-merge M */
static int g_netsolve = 0, g_netsolve_to = 0, g_netsolve_band = 1, g_netsolve_level = 0, g_netsolve_merge = -1, g_netsolve_max_iter = 0;   /* --netsolve FROM, --netsolve-to TO, ... */
static double g_netsolve_rtol = 1e-8;
static int g_netsolve_opts = 0;
static int g_drainage = 0, g_drainage_to = 0, g_drainage_band = 1, g_drainage_plane = 0;   /* --drainage FROM, --drainage-to TO, --drainage-band N, --drainage-plane */
static int g_drainage_to_set = 0;
static int g_geodesic = 0, g_geodesic_to = 0, g_geodesic_band = 1, g_geodesic_conn = 8, g_geodesic_min_d2 = 0, g_geodesic_plane = 0;   /* --geodesic FROM, --geodesic-to TO, --geodesic-band N, --geodesic-conn 4|8, --geodesic-min-d2 D, --geodesic-plane */
static int g_geodesic_opts = 0;   /* one of the options that need --geodesic FROM has been given */
static int g_tracers = 0, g_tracers_nx = 0, g_tracers_ny = 0;   /* --tracers NXxNY */
static int g_dye = 0, g_dye_box[4] = {0, 0, 0, 0};   /* --dye X0,Y0,X1,Y1 */
static double g_dye_tau = 0.53;                      /* --dye-tau T */
static int g_mean = 0;           /* --mean [EVERY] */
static int g_coarse = 0, g_coarse_cw = 0, g_coarse_ch = 0;   /* --coarse CWxCH */
static int g_async_frames = 0;   /* --async-output [N] */
static int g_async_dem = 0;      /* --async-dem [N] */
static int g_async_ckpt = 0;     /* --async-checkpoint [N] */
static long g_ckpt_every = 0;    /* --checkpoint-every N */
static int g_ckpt_state = 0;     /* --checkpoint-state */
/* the optional count behind --async-output: all digits */
static int is_count(const char* s) {
  if (!s || !*s) return 0;
  for (; *s; ++s) if (*s < '0' || *s > '9') return 0;
  return 1;
}
/* the sides behind --drainage and --drainage-to: letters out of BTLR -> B 1 | T 2 | L 4 | R 8, 0 for anything else */
static int side_mask(const char* s) {
  static const char letters[] = "BTLR";
  int mask = 0;
  if (!s || !*s) return 0;
  for (; *s; ++s) {
    const char* at = strchr(letters, *s);
    if (!at) return 0;
    mask |= 1 << (int)(at - letters);
  }
  return mask;
}
static int is_number(const char* s, double* v) {   /* the whole of s is one finite number */
  char* end = NULL;
  if (!s || !*s) return 0;
  *v = strtod(s, &end);
  return end && !*end && *v == *v && *v - *v == 0.;
}
static char g_iddir[256] = "";
static double g_comm_timeout = 180.;   /* seconds the ranks' transport may take to come up (--comm-timeout, LBMDEM_COMM_TIMEOUT) */
static int g_devices[64], g_ndevices = 0;   /* --devices */

/* --probes: the records the library holds are appended to the file, the ring is emptied */
static lbmdem_handle* g_probe_handle = NULL;
static FILE* g_probe_file = NULL;
static long g_probe_records = 0;
static int drain_probes(void) {
  lbmdem_handle* h = g_probe_handle;
  long count = 0, dropped = 0, off[6];
  if (lbmdem_probe_read(h, NULL, 0, &count, &dropped) != LBMDEM_OK || lbmdem_probe_layout(h, off) != LBMDEM_OK) return -1;
  if (count == 0) return 0;
  const long rec = lbmdem_probe_record_doubles(h);
  double* buf = (double*)malloc(sizeof(double) * (size_t)rec * (size_t)count);
  if (!buf || lbmdem_probe_read(h, buf, count, &count, &dropped) != LBMDEM_OK) { free(buf); return -1; }
  if (dropped > 0) fprintf(stderr, "--probes: %ld samples found the ring full and were dropped\n", dropped);
  lbmdem_config cfg;
  if (lbmdem_get_config(h, &cfg) != LBMDEM_OK) { free(buf); return -1; }
  const long npoints = off[4] < 0 ? 0 : (off[5] < 0 ? rec : off[5]) - off[4];
  for (long k = 0; k < count; ++k, ++g_probe_records) {
    const double* R = buf + k * rec;
    fprintf(g_probe_file, "%ld %le %le %le", (long)R[0], R[1], R[off[5]], R[off[5] + 1]);
    for (long j = 0; j < npoints; ++j) fprintf(g_probe_file, " %le", R[off[4] + j]);
    fprintf(g_probe_file, "\n");
    if (off[1] >= 0) {
      char name[64];
      snprintf(name, sizeof name, "pressure_base%.6i.dat", (int)g_probe_records);
      FILE* fp = fopen(name, "w");
      if (!fp) { free(buf); return -1; }
      const double pasxyz = 1. / cfg.lx;   /* main.c:495 */
      for (int x = 0; x < cfg.lx; ++x) fprintf(fp, "%le %le\n", x * pasxyz, R[off[1] + x]);   /* main.c:532 */
      fclose(fp);
    }
  }
  fflush(g_probe_file);
  free(buf);
  return 0;
}
/* The console lines of lbmdem_run_scene, as it prints them itself. The ring is emptied at check_density's line only
 * (main.c:1259): there the library has just synchronised for the serial density sum, so the read costs no stop of its own;
 * the "steps" line is printed without one and is left alone. check_density's line comes when s % npDEM == 0 && s % 400 == 0,
 * i.e. every 400 / gcd(npDEM, 400) fluid steps, 400 at the most: PROBE_RING_RECORDS holds them all for any --probe-every. */
#define PROBE_RING_RECORDS 512
static void say_and_drain(void* user, const char* line) {
  (void)user;
  fputs(line, stdout);
  if (strncmp(line, "Iteration Number", 16) != 0) return;
  if (drain_probes() != 0) { fprintf(stderr, "probe_read: %s\n", lbmdem_last_error()); exit(EXIT_FAILURE); }
}

static int share_id(unsigned char* id) {
  char path[320], tmp[340];
  snprintf(path, sizeof path, "%s/rccl_id", g_iddir);
  if (g_rank == 0) {
    if (lbmdem_comm_unique_id(id) != LBMDEM_OK) return -1;
    if (g_world == 1) return 0;
    snprintf(tmp, sizeof tmp, "%s.tmp", path);
    FILE* fp = fopen(tmp, "wb");
    if (!fp || fwrite(id, 1, LBMDEM_COMM_ID_BYTES, fp) != LBMDEM_COMM_ID_BYTES) return -1;
    fclose(fp);
    return rename(tmp, path);
  }
  for (int tries = 0; tries < 6000; ++tries) { /* up to 60 s */
    FILE* fp = fopen(path, "rb");
    if (fp) {
      size_t got = fread(id, 1, LBMDEM_COMM_ID_BYTES, fp);
      fclose(fp);
      if (got == LBMDEM_COMM_ID_BYTES) return 0;
    }
    usleep(10000);
  }
  return -1;
}

static int run(int argc, char** argv);

static int check_decomposition(int argc, char** argv, int gpus) {
  int lx = 7826, ly = 2325;
  double scale = 1.;
  const char* sample = NULL;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--lx") && a + 1 < argc) lx = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--ly") && a + 1 < argc) ly = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--scale") && a + 1 < argc) scale = atof(argv[++a]);
    else if (argv[a][0] == '-' && argv[a][1] == '-' && strcmp(argv[a], "--comm") && strcmp(argv[a], "--dry") &&
             strcmp(argv[a], "--vib") && strcmp(argv[a], "--run-stats") && strcmp(argv[a], "--async-output") && strcmp(argv[a], "--async-dem") && strcmp(argv[a], "--async-checkpoint") && strcmp(argv[a], "--mean") && a + 1 < argc) ++a;
    else if (argv[a][0] != '-' && !sample) sample = argv[a];
  }
  if (!sample) return 0;   /* run() prints the usage line */
  int n = 0;
  double *r = NULL, *x1 = NULL, *x2 = NULL;
  if (lbmdem_read_sample(sample, &n, &r, &x1, &x2) != LBMDEM_OK) { fprintf(stderr, "read_sample: %s\n", lbmdem_last_error()); return EXIT_FAILURE; }
  lbmdem_config cfg;
  memset(&cfg, 0, sizeof cfg);
  lbmdem_physics_defaults(&cfg.phys);
  if (lbmdem_derive(&cfg, lx, ly, scale, n, r) != LBMDEM_OK) { fprintf(stderr, "derive: %s\n", lbmdem_last_error()); return EXIT_FAILURE; }
  double rmax = r[0];
  for (int i = 1; i < n; ++i) rmax = fmax(rmax, r[i]);
  lbmdem_free_host(r); lbmdem_free_host(x1); lbmdem_free_host(x2);
  const int margin = lbmdem_dist_margin_for(&cfg, rmax);
  int narrowest = lx;
  for (int k = 0; k < gpus; ++k) {
    int w = (int)((long)(k + 1) * lx / gpus) - (int)((long)k * lx / gpus);
    if (w < narrowest) narrowest = w;
  }
  if (narrowest < margin) {
    fprintf(stderr, "--gpus %d: strips of %d rows are narrower than the margin of %d rows this packing needs "
                    "(npDEM = %d sub-steps per fluid step); use at most %d GPUs for a lattice %d rows long\n",
            gpus, narrowest, margin, cfg.npDEM, lx / margin, lx);
    return EXIT_FAILURE;
  }
  return 0;
}

int main(int argc, char** argv) {
  int gpus = 1, probes = 0;
  if (getenv("LBMDEM_COMM_TIMEOUT")) g_comm_timeout = atof(getenv("LBMDEM_COMM_TIMEOUT"));
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--gpus") && a + 1 < argc) gpus = atoi(argv[a + 1]);
    if (!strcmp(argv[a], "--comm")) g_use_comm = 1;   /* the RCCL path with a single rank */
    if (!strcmp(argv[a], "--dry")) g_dry = 1;
    if (!strcmp(argv[a], "--vib")) g_vib = 1;
    if (!strcmp(argv[a], "--contacts")) g_contacts = 1;
    if (!strcmp(argv[a], "--flow")) g_flow = 1;
    if (!strcmp(argv[a], "--clusters")) {
      double k = 1.;
      g_clusters = 1;
      if (a + 1 < argc && is_number(argv[a + 1], &k)) {
        if (k < 0) { fprintf(stderr, "--clusters [K]: the threshold in units of the mean normal force, K at least 0\n"); return EXIT_FAILURE; }
        g_clusters_fmin = k; g_clusters_rel = 1;
      }
    }
    if (!strcmp(argv[a], "--clusters-abs")) {
      double f = 0.;
      if (a + 1 >= argc || !is_number(argv[a + 1], &f) || f < 0) { fprintf(stderr, "--clusters-abs F: the threshold as a force, F at least 0\n"); return EXIT_FAILURE; }
      g_clusters = 1; g_clusters_fmin = f; g_clusters_rel = 0;
    }
    if (!strcmp(argv[a], "--clusters-zmin")) {
      if (a + 1 >= argc || !is_count(argv[a + 1]) || atoi(argv[a + 1]) > 6) { fprintf(stderr, "--clusters-zmin Z: the contacts a grain of the core keeps, 0 .. 6\n"); return EXIT_FAILURE; }
      g_clusters = 1; g_clusters_zmin = atoi(argv[a + 1]);
    }
    if (!strcmp(argv[a], "--structure")) {
      if (a + 1 >= argc || !is_number(argv[a + 1], &g_structure_rcut) || !(g_structure_rcut > 0)) { fprintf(stderr, "--structure RCUT: the neighbours' cutoff in metres, above 0\n"); return EXIT_FAILURE; }
      g_structure = 1;
    }
    if (!strcmp(argv[a], "--voronoi")) {
      if (a + 1 >= argc || !is_number(argv[a + 1], &g_voronoi_rcut) || !(g_voronoi_rcut > 0)) { fprintf(stderr, "--voronoi RCUT: the neighbours' cutoff in metres, above 0\n"); return EXIT_FAILURE; }
      g_voronoi = 1;
    }
    if (!strcmp(argv[a], "--strain")) {
      if (a + 1 >= argc || !is_number(argv[a + 1], &g_strain_rcut) || !(g_strain_rcut > 0)) { fprintf(stderr, "--strain RCUT: the neighbours' cutoff in metres, above 0\n"); return EXIT_FAILURE; }
      g_strain = 1;
    }
    if (!strcmp(argv[a], "--strain-incremental")) g_strain_incremental = 1;
    if (!strcmp(argv[a], "--pores")) {
      g_pores = 1;
      if (a + 1 < argc && is_count(argv[a + 1])) {
        g_pores_conn = atoi(argv[a + 1]);
        if (g_pores_conn != 4 && g_pores_conn != 8) { fprintf(stderr, "--pores [4|8]: the fluid nodes are joined along 4 or 8 directions\n"); return EXIT_FAILURE; }
      }
    }
    if (!strcmp(argv[a], "--pores-plane")) g_pores_plane = 1;
    if (!strcmp(argv[a], "--clearance")) g_clearance = 1;
    if (!strcmp(argv[a], "--clearance-plane")) g_clearance_plane = 1;
    if (!strcmp(argv[a], "--network")) {
      g_network = 1;
      if (a + 1 < argc && is_count(argv[a + 1])) g_network_merge = atoi(argv[a + 1]);
    }
    if (!strcmp(argv[a], "--network-plane")) g_network_plane = 1;
    if (!strcmp(argv[a], "--netflux")) {
      g_netflux = 1;
      if (a + 1 < argc && is_count(argv[a + 1])) g_netflux_level = atoi(argv[a + 1]);
      if (g_netflux_level > 1) { fprintf(stderr, "--netflux [LEVEL]: 0 between the pore bodies, 1 between the merged groups\n"); return EXIT_FAILURE; }
    }
    if (!strcmp(argv[a], "--netflux-merge")) {
      if (a + 1 >= argc || (!is_count(argv[a + 1]) && strcmp(argv[a + 1], "-1"))) { fprintf(stderr, "--netflux-merge M: -1 (no merging) or a difference of radii, 0 or more\n"); return EXIT_FAILURE; }
      g_netflux_merge = atoi(argv[a + 1]); g_netflux_merge_set = 1;
    }
    if (!strcmp(argv[a], "--netsolve") || !strcmp(argv[a], "--netsolve-to")) {
      const int mask = a + 1 < argc ? side_mask(argv[a + 1]) : 0;
      if (mask <= 0) { fprintf(stderr, "%s SIDES: letters out of BTLR, at least one\n", argv[a]); return EXIT_FAILURE; }
      if (!strcmp(argv[a], "--netsolve")) g_netsolve = mask; else { g_netsolve_to = mask; g_netsolve_opts = 1; }
    }
    if (!strcmp(argv[a], "--netsolve-band")) {
      if (a + 1 >= argc || !is_count(argv[a + 1]) || atoi(argv[a + 1]) < 1) { fprintf(stderr, "--netsolve-band N: the depth of the inlet and outlet regions in nodes, at least 1\n"); return EXIT_FAILURE; }
      g_netsolve_band = atoi(argv[a + 1]); g_netsolve_opts = 1;
    }
    if (!strcmp(argv[a], "--netsolve-level")) {
      if (a + 1 >= argc || !is_count(argv[a + 1]) || atoi(argv[a + 1]) > 1) { fprintf(stderr, "--netsolve-level L: 0 between the pore bodies, 1 between the merged groups\n"); return EXIT_FAILURE; }
      g_netsolve_level = atoi(argv[a + 1]); g_netsolve_opts = 1;
    }
    if (!strcmp(argv[a], "--netsolve-merge")) {
      if (a + 1 >= argc || (!is_count(argv[a + 1]) && strcmp(argv[a + 1], "-1"))) { fprintf(stderr, "--netsolve-merge M: -1 (no merging) or a difference of radii, 0 or more\n"); return EXIT_FAILURE; }
      g_netsolve_merge = atoi(argv[a + 1]); g_netsolve_opts = 1;
    }
    if (!strcmp(argv[a], "--netsolve-rtol")) {
      if (a + 1 >= argc || !(atof(argv[a + 1]) > 0.) || !(atof(argv[a + 1]) < 1.)) { fprintf(stderr, "--netsolve-rtol R: the relative residual to stop at, strictly between 0 and 1\n"); return EXIT_FAILURE; }
      g_netsolve_rtol = atof(argv[a + 1]); g_netsolve_opts = 1;
    }
    if (!strcmp(argv[a], "--netsolve-max-iter")) {
      if (a + 1 >= argc || !is_count(argv[a + 1])) { fprintf(stderr, "--netsolve-max-iter K: the most iterations, 0 for the number of free regions\n"); return EXIT_FAILURE; }
      g_netsolve_max_iter = atoi(argv[a + 1]); g_netsolve_opts = 1;
    }
    if (!strcmp(argv[a], "--drainage") || !strcmp(argv[a], "--drainage-to")) {
      const int mask = a + 1 < argc ? side_mask(argv[a + 1]) : 0;
      if (mask <= 0) { fprintf(stderr, "%s SIDES: letters out of BTLR, at least one\n", argv[a]); return EXIT_FAILURE; }
      if (!strcmp(argv[a], "--drainage")) g_drainage = mask; else { g_drainage_to = mask; g_drainage_to_set = 1; }
    }
    if (!strcmp(argv[a], "--drainage-band")) {
      if (a + 1 >= argc || !is_count(argv[a + 1]) || atoi(argv[a + 1]) < 1) { fprintf(stderr, "--drainage-band N: the depth of the reservoir in nodes, at least 1\n"); return EXIT_FAILURE; }
      g_drainage_band = atoi(argv[a + 1]);
    }
    if (!strcmp(argv[a], "--drainage-plane")) g_drainage_plane = 1;
    if (!strcmp(argv[a], "--geodesic") || !strcmp(argv[a], "--geodesic-to")) {
      const int mask = a + 1 < argc ? side_mask(argv[a + 1]) : 0;
      if (mask <= 0) { fprintf(stderr, "%s SIDES: letters out of BTLR, at least one\n", argv[a]); return EXIT_FAILURE; }
      if (!strcmp(argv[a], "--geodesic")) g_geodesic = mask; else { g_geodesic_to = mask; g_geodesic_opts = 1; }
    }
    if (!strcmp(argv[a], "--geodesic-band")) {
      if (a + 1 >= argc || !is_count(argv[a + 1]) || atoi(argv[a + 1]) < 1) { fprintf(stderr, "--geodesic-band N: the depth of the inlet and outlet regions in nodes, at least 1\n"); return EXIT_FAILURE; }
      g_geodesic_band = atoi(argv[a + 1]); g_geodesic_opts = 1;
    }
    if (!strcmp(argv[a], "--geodesic-conn")) {
      if (a + 1 >= argc || (strcmp(argv[a + 1], "4") && strcmp(argv[a + 1], "8"))) { fprintf(stderr, "--geodesic-conn 4|8: the neighbours a path may step to\n"); return EXIT_FAILURE; }
      g_geodesic_conn = atoi(argv[a + 1]); g_geodesic_opts = 1;
    }
    if (!strcmp(argv[a], "--geodesic-min-d2")) {
      if (a + 1 >= argc || !is_count(argv[a + 1])) { fprintf(stderr, "--geodesic-min-d2 D: the least squared clearance of a passable node, 0 or more\n"); return EXIT_FAILURE; }
      g_geodesic_min_d2 = atoi(argv[a + 1]); g_geodesic_opts = 1;
    }
    if (!strcmp(argv[a], "--geodesic-plane")) { g_geodesic_plane = 1; g_geodesic_opts = 1; }
    if (!strcmp(argv[a], "--structure-bins")) {
      if (a + 1 >= argc || !is_count(argv[a + 1]) || atoi(argv[a + 1]) < 1 || atoi(argv[a + 1]) > 4096) { fprintf(stderr, "--structure-bins N: the bins of the pair histogram, 1 .. 4096\n"); return EXIT_FAILURE; }
      g_structure_bins = atoi(argv[a + 1]);
    }
    if (!strcmp(argv[a], "--structure-shell")) {
      if (a + 1 >= argc || !is_number(argv[a + 1], &g_structure_shell) || !(g_structure_shell >= 1)) { fprintf(stderr, "--structure-shell S: a bond reaches S times the sum of two radii, S at least 1\n"); return EXIT_FAILURE; }
    }
    if (!strcmp(argv[a], "--coarse")) {
      char tail = 0;
      if (a + 1 >= argc || sscanf(argv[a + 1], "%dx%d%c", &g_coarse_cw, &g_coarse_ch, &tail) != 2 || g_coarse_cw < 1 || g_coarse_ch < 1) {
        fprintf(stderr, "--coarse CWxCH: lattice nodes per cell in x and y, both at least 1 (16x16)\n");
        return EXIT_FAILURE;
      }
      g_coarse = 1;
    }
    if (!strcmp(argv[a], "--tracers")) {
      char tail = 0;
      if (a + 1 >= argc || sscanf(argv[a + 1], "%dx%d%c", &g_tracers_nx, &g_tracers_ny, &tail) != 2 || g_tracers_nx < 1 || g_tracers_ny < 1 ||
          (long)g_tracers_nx * g_tracers_ny > 16777216L) {
        fprintf(stderr, "--tracers NXxNY: tracers along x and y, both at least 1, at most 2^24 in all (256x256)\n");
        return EXIT_FAILURE;
      }
      g_tracers = 1;
    }
    if (!strcmp(argv[a], "--dye")) {
      char tail = 0;
      if (a + 1 >= argc || sscanf(argv[a + 1], "%d,%d,%d,%d%c", &g_dye_box[0], &g_dye_box[1], &g_dye_box[2], &g_dye_box[3], &tail) != 4 ||
          g_dye_box[0] < 0 || g_dye_box[1] < 0 || g_dye_box[2] < g_dye_box[0] || g_dye_box[3] < g_dye_box[1]) {
        fprintf(stderr, "--dye X0,Y0,X1,Y1: a box of nodes, 0 <= X0 <= X1 and 0 <= Y0 <= Y1\n");
        return EXIT_FAILURE;
      }
      g_dye = 1;
    }
    if (!strcmp(argv[a], "--dye-tau")) {
      char tail = 0;
      if (a + 1 >= argc || sscanf(argv[a + 1], "%lf%c", &g_dye_tau, &tail) != 1 || !(g_dye_tau > 0.5)) {
        fprintf(stderr, "--dye-tau T: the relaxation time of the dye, larger than 0.5\n");
        return EXIT_FAILURE;
      }
    }
    if (!strcmp(argv[a], "--mean")) {
      g_mean = (a + 1 < argc && is_count(argv[a + 1])) ? atoi(argv[a + 1]) : 1;
      if (g_mean < 1) { fprintf(stderr, "--mean [EVERY]: every EVERY-th fluid step is sampled, EVERY at least 1\n"); return EXIT_FAILURE; }
    }
    if (!strcmp(argv[a], "--run-stats")) g_run_stats = 1;
    if (!strcmp(argv[a], "--probes")) probes = 1;
    if (!strcmp(argv[a], "--dump-geometry") && a + 1 < argc) g_dump_geometry = argv[a + 1];
    if (!strcmp(argv[a], "--densities") && a + 1 < argc) g_densities = argv[a + 1];
    if (!strcmp(argv[a], "--async-output")) g_async_frames = (a + 1 < argc && is_count(argv[a + 1])) ? atoi(argv[a + 1]) : 2;
    if (!strcmp(argv[a], "--async-dem")) g_async_dem = (a + 1 < argc && is_count(argv[a + 1])) ? atoi(argv[a + 1]) : 2;
    if (!strcmp(argv[a], "--async-checkpoint")) g_async_ckpt = (a + 1 < argc && is_count(argv[a + 1])) ? atoi(argv[a + 1]) : 1;
    if (!strcmp(argv[a], "--checkpoint-every") && a + 1 < argc) g_ckpt_every = atol(argv[a + 1]);
    if (!strcmp(argv[a], "--checkpoint-state")) g_ckpt_state = 1;
    if (!strcmp(argv[a], "--verify-checkpoint") && a + 1 < argc) {   /* host only: no device is touched */
      int has = 0;
      if (lbmdem_checkpoint_verify(argv[a + 1], &has) != LBMDEM_OK) { fprintf(stderr, "verify-checkpoint: %s\n", lbmdem_last_error()); return EXIT_FAILURE; }
      printf("%s: %s\n", argv[a + 1], has ? "every section matches its digest" : "no digests (written by lbmdem_checkpoint_save)");
      return 0;
    }
    if (!strcmp(argv[a], "--comm-timeout") && a + 1 < argc) g_comm_timeout = atof(argv[a + 1]);
    if (!strcmp(argv[a], "--devices") && a + 1 < argc) {
      for (const char* p = argv[a + 1]; *p && g_ndevices < 64;) {
        char* end = NULL;
        long v = strtol(p, &end, 10);
        if (end == p || v < 0) { fprintf(stderr, "--devices: a comma-separated list of device ordinals\n"); return EXIT_FAILURE; }
        g_devices[g_ndevices++] = (int)v;
        p = (*end == ',') ? end + 1 : end;
        if (*end && *end != ',') { fprintf(stderr, "--devices: a comma-separated list of device ordinals\n"); return EXIT_FAILURE; }
      }
    }
  }
  if (g_ndevices > 0 && g_ndevices < gpus) { fprintf(stderr, "--devices names %d devices for %d ranks\n", g_ndevices, gpus); return EXIT_FAILURE; }
  if (g_dry && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--dry is a single-GPU mode (the strips exist for the fluid)\n"); return EXIT_FAILURE; }
  if (g_vib && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--vib is a single-GPU mode (vibrating walls are not available on strips)\n"); return EXIT_FAILURE; }
  if (probes && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--probes is a single-GPU mode (the probes are not available on strips)\n"); return EXIT_FAILURE; }
  if (g_dump_geometry && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--dump-geometry is a single-GPU mode (the boundary-link export needs the whole lattice on one handle)\n"); return EXIT_FAILURE; }
  if (g_densities && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--densities is a single-GPU mode (write_densities needs the whole lattice on one handle)\n"); return EXIT_FAILURE; }
  if (g_contacts && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--contacts is a single-GPU mode (the contact network export needs all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_coarse && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--coarse is a single-GPU mode (the coarse-grained fields need the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_clusters && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--clusters is a single-GPU mode (the cluster analysis needs all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_structure && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--structure is a single-GPU mode (the packing structure analysis needs all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_strain && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--strain is a single-GPU mode (the strain analysis needs all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_strain_incremental && !g_strain) { fprintf(stderr, "--strain-incremental goes with --strain RCUT\n"); return EXIT_FAILURE; }
  if (g_voronoi && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--voronoi is a single-GPU mode (the Voronoi analysis needs all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_pores_plane && !g_pores) { fprintf(stderr, "--pores-plane needs --pores\n"); return EXIT_FAILURE; }
  if (g_pores && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--pores is a single-GPU mode (the pore space analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_pores && g_dry) { fprintf(stderr, "--pores cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_clearance_plane && !g_clearance) { fprintf(stderr, "--clearance-plane needs --clearance\n"); return EXIT_FAILURE; }
  if (g_clearance && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--clearance is a single-GPU mode (the pore clearance analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_clearance && g_dry) { fprintf(stderr, "--clearance cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_network_plane && !g_network) { fprintf(stderr, "--network-plane needs --network\n"); return EXIT_FAILURE; }
  if (g_network && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--network is a single-GPU mode (the pore network analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_netflux_merge_set && !g_netflux) { fprintf(stderr, "--netflux-merge needs --netflux\n"); return EXIT_FAILURE; }
  if (g_netflux && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--netflux is a single-GPU mode (the pore flux analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_netflux && g_dry) { fprintf(stderr, "--netflux cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_network && g_dry) { fprintf(stderr, "--network cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_netsolve_opts && !g_netsolve) { fprintf(stderr, "--netsolve-to, --netsolve-band, --netsolve-level, --netsolve-merge, --netsolve-rtol and --netsolve-max-iter need --netsolve FROM\n"); return EXIT_FAILURE; }
  if (g_netsolve && !g_netsolve_to) { fprintf(stderr, "--netsolve FROM needs --netsolve-to TO\n"); return EXIT_FAILURE; }
  if (g_netsolve && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--netsolve is a single-GPU mode (the network pressure analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_netsolve && g_dry) { fprintf(stderr, "--netsolve cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if ((g_drainage_plane || g_drainage_to_set || g_drainage_band != 1) && !g_drainage) { fprintf(stderr, "--drainage-to, --drainage-band and --drainage-plane need --drainage FROM\n"); return EXIT_FAILURE; }
  if (g_drainage && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--drainage is a single-GPU mode (the drainage analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_drainage && g_dry) { fprintf(stderr, "--drainage cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_geodesic_opts && !g_geodesic) { fprintf(stderr, "--geodesic-to, --geodesic-band, --geodesic-conn, --geodesic-min-d2 and --geodesic-plane need --geodesic FROM\n"); return EXIT_FAILURE; }
  if (g_geodesic && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--geodesic is a single-GPU mode (the geodesic analysis needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_geodesic && g_dry) { fprintf(stderr, "--geodesic cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_flow && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--flow is a single-GPU mode (the flow fields need the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_tracers && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--tracers is a single-GPU mode (the tracers need the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_dye && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--dye is a single-GPU mode (the passive scalar needs the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_mean && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--mean is a single-GPU mode (the time-averaged statistics need the whole lattice and all grains on one handle)\n"); return EXIT_FAILURE; }
  if (g_mean && g_dry) { fprintf(stderr, "--mean cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_dye && g_dry) { fprintf(stderr, "--dye cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_tracers && g_dry) { fprintf(stderr, "--tracers cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_flow && g_dry) { fprintf(stderr, "--flow cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_densities && g_dry) { fprintf(stderr, "--densities cannot be combined with --dry (there is no fluid)\n"); return EXIT_FAILURE; }
  if (g_async_frames && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--async-output is a single-GPU mode (with --gpus N rank 0 merges the strips' columns and writes the frames itself)\n"); return EXIT_FAILURE; }
  if (g_async_dem && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--async-dem is a single-GPU mode (with --gpus N rank 0 runs the table sub-step on a full replica and writes the tables itself)\n"); return EXIT_FAILURE; }
  if ((g_async_ckpt || g_ckpt_every) && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--checkpoint-every and --async-checkpoint are single-GPU modes (with --gpus N every rank saves its own file at the end)\n"); return EXIT_FAILURE; }
  if (g_ckpt_every < 0) { fprintf(stderr, "--checkpoint-every N: a number of DEM steps\n"); return EXIT_FAILURE; }
  if (g_ckpt_state && (gpus > 1 || g_use_comm)) { fprintf(stderr, "--checkpoint-state is a single-GPU mode (a strip's checkpoint holds the strip and nothing else)\n"); return EXIT_FAILURE; }
  if (gpus <= 1) return run(argc, argv);
  g_world = gpus; g_use_comm = 1;
  { /* every strip must be at least one margin wide (lbmdem_dist_enable would refuse on the ranks whose strip is one
     * row narrower, and the others would wait for them): checked here, on the host, before anything is forked */
    int rc = check_decomposition(argc, argv, gpus);
    if (rc != 0) return rc;
  }
  snprintf(g_iddir, sizeof g_iddir, "/tmp/lbmdem_XXXXXX");
  if (!mkdtemp(g_iddir)) { perror("mkdtemp"); return EXIT_FAILURE; }
  pid_t pids[64];
  if (gpus > 64) { fprintf(stderr, "--gpus: at most 64\n"); return EXIT_FAILURE; }
  for (int r = 0; r < gpus; ++r) {
    pids[r] = fork();
    if (pids[r] < 0) { perror("fork"); return EXIT_FAILURE; }
    if (pids[r] == 0) {   /* (_exit does not flush: into a pipe or a file the end of rank 0's console lines was lost) */
      g_rank = r;
      int rc = run(argc, argv);
      fflush(stdout);
      _exit(rc);
    }
  }
  /* the first rank that fails takes the others with it: its peers would otherwise block for ever inside an RCCL call */
  int bad = 0, left = gpus;
  /* ... and so does a transport that never comes up (a rank stuck in communicator creation or in its first exchange
   * with a neighbour cannot report anything): every rank leaves a file once lbmdem_comm_selftest has passed; ranks that
   * have not all done so after --comm-timeout seconds (default 180; LBMDEM_COMM_TIMEOUT) are killed with a message
   * instead of hanging the job. bench.py guards its C driver the same way (a watchdogged trial). */
  {
    const double limit = g_comm_timeout;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    int up = 0;
    while (left > 0 && !bad && !up && limit > 0) {
      int st = 0;
      pid_t p = waitpid(-1, &st, WNOHANG);
      if (p > 0) {
        --left;
        for (int r = 0; r < gpus; ++r) if (pids[r] == p) pids[r] = 0;
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
          for (int r = 0; r < gpus; ++r) if (pids[r] > 0) kill(pids[r], SIGKILL);
          bad = 1;
        }
        continue;
      }
      up = 1;
      for (int r = 0; r < gpus && up; ++r) {
        char f[320];
        snprintf(f, sizeof f, "%s/up.%d", g_iddir, r);
        if (access(f, F_OK) != 0) up = 0;
      }
      if (up) break;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > limit) {
        fprintf(stderr, "--gpus %d: the ranks' transport (RCCL communicators + a first exchange with both neighbours) did not "
                        "come up within %.0f s: stopping all ranks (--comm-timeout S / LBMDEM_COMM_TIMEOUT to wait longer)\n",
                gpus, limit);
        for (int r = 0; r < gpus; ++r) if (pids[r] > 0) kill(pids[r], SIGKILL);
        bad = 1;
        break;
      }
      struct timespec nap = {0, 20 * 1000 * 1000};
      nanosleep(&nap, NULL);
    }
  }
  while (left > 0) {
    int st = 0;
    pid_t p = waitpid(-1, &st, 0);
    if (p < 0) break;
    --left;
    for (int r = 0; r < gpus; ++r) if (pids[r] == p) pids[r] = 0;
    if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
      if (!bad) for (int r = 0; r < gpus; ++r) if (pids[r] > 0) kill(pids[r], SIGKILL);
      bad = 1;
    }
  }
  char path[320];
  for (int r = 0; r < gpus; ++r) { snprintf(path, sizeof path, "%s/up.%d", g_iddir, r); unlink(path); }
  snprintf(path, sizeof path, "%s/rccl_id", g_iddir); unlink(path); rmdir(g_iddir);
  return bad ? EXIT_FAILURE : 0;
}

#define SAY(...) do { if (g_rank == 0) printf(__VA_ARGS__); } while (0)

/* check_density / final_density with the reference's own bits (main.c:1249-1273): ONE serial chain over the whole
 * lattice. With several strips the chain runs through the ranks in x order: rank r continues from rank r-1's sum
 * (handed on through the all-reduce: everybody else contributes 0). Every rank returns the lattice's sum. */
static double serial_density(lbmdem_handle* h, lbmdem_comm* comm) {
  double s = 0.;
  for (int r = 0; r < g_world; ++r) {
    double v = 0.;
    if (r == g_rank && lbmdem_total_density_serial(h, s, &v, NULL) != LBMDEM_OK) {
      fprintf(stderr, "total_density_serial: %s\n", lbmdem_last_error());
      exit(EXIT_FAILURE);
    }
    if (comm && lbmdem_comm_allreduce_sum(comm, &v, 1) != LBMDEM_OK) {
      fprintf(stderr, "allreduce: %s\n", lbmdem_last_error());
      exit(EXIT_FAILURE);
    }
    s = v;
  }
  return s;
}

/* --run-stats: the line of one kind of background job (lbmdem_output_stats*: `last` is what the kind's fourth time means) */
static int print_async_stats(lbmdem_handle* h, int (*stats)(lbmdem_handle*, long*, double*), const char* label, const char* last) {
  long oc[4];
  double oms[4];
  const int rc = stats(h, oc, oms);
  if (rc == LBMDEM_OK)
    fprintf(stderr, "%s: queued %ld written %ld failed %ld slot_waits %ld ms_slot_wait %.3f ms_copy_wait %.3f ms_io %.3f %s %.3f\n",
            label, oc[0], oc[1], oc[2], oc[3], oms[0], oms[1], oms[2], last, oms[3]);
  return rc;
}

static int run(int argc, char** argv) {
  int lx = 7826, ly = 2325, device = 0; /* main.c:27-32 */
  double scale = 1., duration = 1.5;   /* main.c:24-26,47 */
  long max_steps = -1;
  const char* sample = NULL;
  const char *ckpt_out = NULL, *ckpt_in = NULL;
  double vib_freq = -1., vib_amp = -1.;   /* --vib-freq, --vib-amp (negative: the reference's initialisers) */
  const char* probe_path = NULL;          /* --probes */
  int probe_every = 1, probe_row = 2, probe_points[2 * LBMDEM_PROBE_MAX_POINTS], probe_npoints = 0;
  /* device-resident kernel arguments: ~1.2 us less per launch (the HIP runtime reads this when it
   * initialises, i.e. at the first lbmdem_* call below); an explicit setting of the caller wins */
  setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
  SAY("2D LBM-DEM code\n");
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--lx") && a + 1 < argc) lx = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--ly") && a + 1 < argc) ly = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--scale") && a + 1 < argc) scale = atof(argv[++a]);
    else if (!strcmp(argv[a], "--duration") && a + 1 < argc) duration = atof(argv[++a]);
    else if (!strcmp(argv[a], "--steps") && a + 1 < argc) max_steps = atol(argv[++a]);
    else if (!strcmp(argv[a], "--device") && a + 1 < argc) device = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--checkpoint") && a + 1 < argc) ckpt_out = argv[++a];
    else if (!strcmp(argv[a], "--restart") && a + 1 < argc) ckpt_in = argv[++a];
    else if (!strcmp(argv[a], "--gpus") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--comm-timeout") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--devices") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--comm")) {}
    else if (!strcmp(argv[a], "--dry")) {}
    else if (!strcmp(argv[a], "--vib")) {}
    else if (!strcmp(argv[a], "--contacts")) {}
    else if (!strcmp(argv[a], "--flow")) {}
    else if (!strcmp(argv[a], "--clusters")) { double k; if (a + 1 < argc && is_number(argv[a + 1], &k)) ++a; }
    else if (!strcmp(argv[a], "--clusters-abs") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--clusters-zmin") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--structure") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--voronoi") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--strain") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--strain-incremental")) {}
    else if (!strcmp(argv[a], "--pores")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--pores-plane")) {}
    else if (!strcmp(argv[a], "--clearance")) {}
    else if (!strcmp(argv[a], "--clearance-plane")) {}
    else if (!strcmp(argv[a], "--network")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--network-plane")) {}
    else if (!strcmp(argv[a], "--netflux")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--netflux-merge") && a + 1 < argc) ++a;
    else if ((!strcmp(argv[a], "--netsolve") || !strcmp(argv[a], "--netsolve-to") || !strcmp(argv[a], "--netsolve-band") || !strcmp(argv[a], "--netsolve-level") || !strcmp(argv[a], "--netsolve-merge") || !strcmp(argv[a], "--netsolve-rtol") || !strcmp(argv[a], "--netsolve-max-iter")) && a + 1 < argc) ++a;
    else if ((!strcmp(argv[a], "--drainage") || !strcmp(argv[a], "--drainage-to") || !strcmp(argv[a], "--drainage-band")) && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--drainage-plane")) {}
    else if ((!strcmp(argv[a], "--geodesic") || !strcmp(argv[a], "--geodesic-to") || !strcmp(argv[a], "--geodesic-band") || !strcmp(argv[a], "--geodesic-conn") || !strcmp(argv[a], "--geodesic-min-d2")) && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--geodesic-plane")) {}
    else if (!strcmp(argv[a], "--structure-bins") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--structure-shell") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--coarse") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--tracers") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--dye") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--dye-tau") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--mean")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--run-stats")) {}
    else if (!strcmp(argv[a], "--async-output")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--async-dem")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--async-checkpoint")) { if (a + 1 < argc && is_count(argv[a + 1])) ++a; }
    else if (!strcmp(argv[a], "--checkpoint-every") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--checkpoint-state")) {}
    else if (!strcmp(argv[a], "--vib-freq") && a + 1 < argc) vib_freq = atof(argv[++a]);
    else if (!strcmp(argv[a], "--vib-amp") && a + 1 < argc) vib_amp = atof(argv[++a]);
    else if (!strcmp(argv[a], "--probes") && a + 1 < argc) probe_path = argv[++a];
    else if (!strcmp(argv[a], "--dump-geometry") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--densities") && a + 1 < argc) ++a;
    else if (!strcmp(argv[a], "--probe-every") && a + 1 < argc) probe_every = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--probe-row") && a + 1 < argc) probe_row = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--probe-point") && a + 1 < argc) {
      int px = 0, py = 0;
      if (probe_npoints >= LBMDEM_PROBE_MAX_POINTS || sscanf(argv[++a], "%d,%d", &px, &py) != 2) {
        fprintf(stderr, "--probe-point X,Y: a lattice node, at most %d of them\n", LBMDEM_PROBE_MAX_POINTS);
        return EXIT_FAILURE;
      }
      probe_points[2 * probe_npoints] = px; probe_points[2 * probe_npoints + 1] = py; ++probe_npoints;
    }
    else if (argv[a][0] != '-' && !sample) sample = argv[a];
    else { sample = NULL; break; }
  }
  if (!sample) {
    SAY("usage: usage %s <filename> [--lx N --ly N --scale S --duration T --steps N --device K --gpus N --devices a,b,.. --comm-timeout S --dry --vib --vib-freq F --vib-amp A --run-stats --async-output [N] --async-dem [N] --checkpoint FILE --restart FILE --checkpoint-every N --checkpoint-state --async-checkpoint [N] --verify-checkpoint FILE --probes FILE --probe-every K --probe-row Y --probe-point X,Y --dump-geometry DIR --densities DIR --contacts --clusters [K] --clusters-abs F --clusters-zmin Z --structure RCUT --structure-bins N --structure-shell S --voronoi RCUT --strain RCUT --strain-incremental --pores [4|8] --pores-plane --clearance --clearance-plane --network [MERGE] --network-plane --netflux [LEVEL] --netflux-merge M --netsolve FROM --netsolve-to TO --netsolve-band N --netsolve-level L --netsolve-merge M --netsolve-rtol R --netsolve-max-iter K --drainage FROM --drainage-to TO --drainage-band N --drainage-plane --geodesic FROM --geodesic-to TO --geodesic-band N --geodesic-conn 4|8 --geodesic-min-d2 D --geodesic-plane --coarse CWxCH --flow --tracers NXxNY --dye X0,Y0,X1,Y1 --dye-tau T --mean [EVERY]]\n", argv[0]);
    exit(EXIT_FAILURE);
  }
  if (g_ckpt_every > 0 && !ckpt_out) { fprintf(stderr, "--checkpoint-every needs --checkpoint FILE\n"); return EXIT_FAILURE; }
  SAY("Opening file : %s\n", sample);

  int n = 0;
  double *r = NULL, *x1 = NULL, *x2 = NULL;
  DIE(lbmdem_read_sample(sample, &n, &r, &x1, &x2), "read_sample");
  SAY("Nb grains %d\n", n);
  { /* check_sample, main.c:640-658 */
    double xMax = x1[0], xMin = x1[0], yMax = x2[0], yMin = x2[0], mass = 0.;
    for (int i = 0; i < n; ++i) {
      mass += 2650 * 3.14159265358979 * r[i] * r[i];
      xMax = fmax(xMax, x1[i] + r[i]); xMin = fmin(xMin, x1[i] - r[i]);
      yMax = fmax(yMax, x2[i] + r[i]); yMin = fmin(yMin, x2[i] - r[i]);
    }
    double L0 = xMax - xMin, H0 = yMax - yMin;
    SAY("L0=%le H0=%le Mass of Grains=%le Phi=%le\n", L0, H0, mass, mass / (2650 * (L0 * H0)));
  }

  lbmdem_config cfg;
  memset(&cfg, 0, sizeof cfg);
  DIE(lbmdem_physics_defaults(&cfg.phys), "physics_defaults");
  if (vib_freq >= 0.) cfg.phys.freq = vib_freq;
  if (vib_amp >= 0.) cfg.phys.amp = vib_amp;
  DIE(lbmdem_derive(&cfg, lx, ly, scale, n, r), "derive");
  cfg.x_begin = 0; cfg.x_end = lx; cfg.halo = 0; cfg.device = device;
  if (g_use_comm) { /* this rank's strip */
    cfg.x_begin = (int)((long)g_rank * lx / g_world);
    cfg.x_end = (int)((long)(g_rank + 1) * lx / g_world);
    cfg.halo = g_world > 1 ? 2 : 0;
    cfg.device = g_ndevices > 0 ? g_devices[g_rank] : device + g_rank;
  }
  /* with several strips every rank keeps its own checkpoint file: FILE.rank<k> */
  char ckpt_in_rank[4096], ckpt_out_rank[4096];
  if (g_use_comm && ckpt_in) { snprintf(ckpt_in_rank, sizeof ckpt_in_rank, "%s.rank%d", ckpt_in, g_rank); ckpt_in = ckpt_in_rank; }
  if (g_use_comm && ckpt_out) { snprintf(ckpt_out_rank, sizeof ckpt_out_rank, "%s.rank%d", ckpt_out, g_rank); ckpt_out = ckpt_out_rank; }
  SAY("no space %le\n", cfg.dx);
  {
    double rMin = r[0];
    for (int i = 1; i < n; ++i) rMin = fmin(rMin, r[i]);
    double dtmax = (1 / cfg.phys.iterDEM) * 3.14159265358979 * rMin * sqrt(3.14159265358979 * 2650 / cfg.phys.kg);
    SAY("dtLB=%le,  dtmax=%le,   dt=%le,   npDEM=%d,   c=%lf\n", cfg.dtLB, dtmax, cfg.dt, cfg.npDEM, cfg.c);
  }
  lbmdem_handle* h = NULL;
  long nbsteps = 0;
  int got_tracers = 0, got_dye = 0;   /* --restart: the file carried them, and they are not seeded again */
  if (ckpt_in) {
    DIE(lbmdem_checkpoint_load(ckpt_in, cfg.device, &h), "checkpoint_load");
    DIE(lbmdem_get_config(h, &cfg), "get_config");
    if (g_use_comm && (cfg.x_begin != (int)((long)g_rank * cfg.lx / g_world) || cfg.x_end != (int)((long)(g_rank + 1) * cfg.lx / g_world))) {
      fprintf(stderr, "%s holds rows [%d, %d): written by a run with another number of strips\n", ckpt_in, cfg.x_begin, cfg.x_end);
      return EXIT_FAILURE;
    }
    nbsteps = lbmdem_nbsteps(h);
    SAY("Restarted from %s at step %ld\n", ckpt_in, nbsteps);
    if (!g_use_comm) {   /* what of the optional state came back with the file (--checkpoint-state of the run that wrote it) */
      long tr[3], sc[3], mn[5];
      DIE(lbmdem_tracer_stats(h, tr), "tracer_stats");
      DIE(lbmdem_scalar_stats(h, sc), "scalar_stats");
      DIE(lbmdem_mean_stats(h, mn), "mean_stats");
      got_tracers = tr[0] > 0; got_dye = sc[0] != 0;
      if (got_tracers || got_dye || mn[0]) {
        SAY("Restored with it:");
        if (got_tracers) SAY(" %ld tracers (%ld advances)", tr[0], tr[1]);
        if (got_dye) SAY(" the dye (%ld steps)", sc[1]);
        if (mn[0]) SAY(" an averaging window (mask %ld, %ld samples)", mn[1], mn[2]);
        SAY("\n");
      }
    }
  } else {
    DIE(lbmdem_create(&cfg, r, x1, x2, &h), "create");
  }
  if (g_contacts) DIE(lbmdem_set_contacts_output(h, 1), "set_contacts_output");
  if (g_clusters) DIE(lbmdem_set_clusters_output(h, 1, g_clusters_fmin, g_clusters_rel, g_clusters_zmin), "set_clusters_output");
  if (g_structure) DIE(lbmdem_set_structure_output(h, 1, g_structure_rcut, g_structure_bins, g_structure_shell), "set_structure_output");
  if (g_voronoi) DIE(lbmdem_set_voronoi_output(h, 1, g_voronoi_rcut), "set_voronoi_output");
  if (g_strain) DIE(lbmdem_set_strain_output(h, 1, g_strain_rcut, g_strain_incremental), "set_strain_output");
  if (g_pores) DIE(lbmdem_set_pores_output(h, 1, g_pores_conn, g_pores_plane), "set_pores_output");
  if (g_clearance) DIE(lbmdem_set_clearance_output(h, 1, g_clearance_plane), "set_clearance_output");
  if (g_network) DIE(lbmdem_set_network_output(h, 1, g_network_merge, g_network_plane), "set_network_output");
  if (g_netflux) DIE(lbmdem_set_netflux_output(h, 1, g_netflux_merge, g_netflux_level), "set_netflux_output");
  if (g_netsolve) DIE(lbmdem_set_netsolve_output(h, 1, g_netsolve_merge, g_netsolve_level, g_netsolve, g_netsolve_band, g_netsolve_to, g_netsolve_rtol, g_netsolve_max_iter), "set_netsolve_output");
  if (g_drainage) DIE(lbmdem_set_drainage_output(h, 1, g_drainage, g_drainage_band, g_drainage_to, g_drainage_plane), "set_drainage_output");
  if (g_geodesic) DIE(lbmdem_set_geodesic_output(h, 1, g_geodesic, g_geodesic_band, g_geodesic_to, g_geodesic_conn, g_geodesic_min_d2, g_geodesic_plane), "set_geodesic_output");
  if (g_flow) DIE(lbmdem_set_flow_output(h, 1), "set_flow_output");
  if (g_coarse) DIE(lbmdem_set_coarse_output(h, g_coarse_cw, g_coarse_ch), "set_coarse_output");
  if (g_tracers && got_tracers) DIE(lbmdem_set_tracer_output(h, 1), "set_tracer_output");   /* the loaded set goes on: tracer k stays tracer k */
  else if (g_tracers) {   /* a uniform grid over the whole domain; automatic advance, a file per frame */
    const long nt = (long)g_tracers_nx * g_tracers_ny;
    double* xy = (double*)malloc(sizeof(double) * 2 * (size_t)nt);
    if (!xy) { fprintf(stderr, "--tracers: out of memory\n"); return EXIT_FAILURE; }
    for (int i = 0; i < g_tracers_nx; ++i)
      for (int j = 0; j < g_tracers_ny; ++j) {
        xy[2 * ((long)i * g_tracers_ny + j)] = (i + 0.5) * (cfg.lx - 1) / g_tracers_nx;
        xy[2 * ((long)i * g_tracers_ny + j) + 1] = (j + 0.5) * (cfg.ly - 1) / g_tracers_ny;
      }
    DIE(lbmdem_tracer_set(h, nt, xy, 1), "tracer_set");
    free(xy);
    DIE(lbmdem_set_tracer_output(h, 1), "set_tracer_output");
  }
  if (g_dye && got_dye) DIE(lbmdem_set_scalar_output(h, 1), "set_scalar_output");   /* the loaded field goes on */
  else if (g_dye) {   /* C = 1 in the box (cut to the lattice), 0 elsewhere; automatic step, a file per frame, a line per DEM event */
    double* dye = (double*)calloc((size_t)cfg.lx * cfg.ly, sizeof(double));
    if (!dye) { fprintf(stderr, "--dye: out of memory\n"); return EXIT_FAILURE; }
    for (int x = g_dye_box[0]; x <= g_dye_box[2] && x < cfg.lx; ++x)
      for (int y = g_dye_box[1]; y <= g_dye_box[3] && y < cfg.ly; ++y) dye[(size_t)x * cfg.ly + y] = 1.;
    DIE(lbmdem_scalar_set(h, dye, g_dye_tau, 1), "scalar_set");
    free(dye);
    DIE(lbmdem_set_scalar_output(h, 1), "set_scalar_output");
  }
  if (g_mean) DIE(lbmdem_set_mean_output(h, LBMDEM_MEAN_ALL, g_mean), "set_mean_output");   /* (a loaded window with this mask and cadence goes on: lbmdem_run_scene) */
  if (g_ckpt_state) DIE(lbmdem_set_checkpoint_contents(h, LBMDEM_CKPT_ALL), "set_checkpoint_contents");   /* every save below */
  if (g_vib) DIE(lbmdem_set_vibration(h, 1), "set_vibration");   /* (a restarted vibrating run vibrates anyway) */
  if (g_async_frames) DIE(lbmdem_set_async_output(h, g_async_frames), "set_async_output");   /* set-up, like create: before the clock starts */
  if (g_async_dem) DIE(lbmdem_set_async_dem(h, g_async_dem), "set_async_dem");
  if (g_async_ckpt) DIE(lbmdem_set_async_checkpoint(h, g_async_ckpt), "set_async_checkpoint");
  if (g_ckpt_every > 0) DIE(lbmdem_set_checkpoint_every(h, g_ckpt_every, ckpt_out), "set_checkpoint_every");
  lbmdem_comm* comm = NULL;
  if (g_use_comm) {
    unsigned char id[LBMDEM_COMM_ID_BYTES];
    if (share_id(id) != 0) { fprintf(stderr, "rank %d: no RCCL id: %s\n", g_rank, lbmdem_last_error()); return EXIT_FAILURE; }
    if (!ckpt_in) DIE(lbmdem_dist_enable(h, 0), "dist_enable");   /* a restarted strip comes back distributed */
    DIE(lbmdem_comm_create(id, g_rank, g_world, cfg.device, &comm), "comm_create");
    DIE(lbmdem_comm_selftest(comm, 4096), "comm_selftest");   /* one rank: to itself; several: with both neighbours */
    if (g_iddir[0]) {   /* tell the parent that this rank's transport works (its start-up watchdog) */
      char f[320];
      snprintf(f, sizeof f, "%s/up.%d", g_iddir, g_rank);
      FILE* u = fopen(f, "w");
      if (u) fclose(u);
    }
  }
  time_t now = time(NULL);
  SAY("Current local time and date: %s", asctime(localtime(&now)));
  if (!ckpt_in && g_rank == 0) { /* stats.data header, main.c:1867-1877 */
    FILE* st = fopen("stats.data", "w");
    if (st) {
      fprintf(st, "#1_t 2_xfront 3_xgrainmax 4_height 5_zmean 6_energie_x 7_energie_y "
                  "8_energie_teta 9_energie_cin 10_N0 11_N1 12_N2 13_N3 14_N4 15_N5 "
                  "16_energy_Potential 17_Strain_Energy 18_Frictional_Work "
                  "19_Internal_Friction 20_Inelastic_Collision 21_Slip "
                  "22_Rotational_Work\n");
      fclose(st);
    }
  }

  /* main loop, main.c:1879-1890: the library's (lbmdem_run_scene) -- check_density's lines, write_vtk every stepFilm DEM
   * steps, write_DEM / write_forces every 4000, the "steps" line every updateVerlet, the stop test after EVERY renderScene().
   * Between two of those the sub-steps reach the run loop in one piece. With several strips rank 0 prints and writes (the VTK
   * columns merged over the ranks; the sub-step before a write_DEM run by rank 0 on a full replica). */
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  lbmdem_scene scene;
  memset(&scene, 0, sizeof scene);
  scene.dir = ".";
  scene.fluid = !g_dry;   /* --dry: renderScene without its `#ifdef _FLUIDE_` blocks (main.c:1709-1719,1768-1770) */
  scene.duration = duration;
  lbmdem_scene_result done;
  memset(&done, 0, sizeof done);
  if (probe_path) {
    lbmdem_probe_config pc;
    memset(&pc, 0, sizeof pc);
    pc.every = probe_every; pc.capacity = PROBE_RING_RECORDS; pc.pressure_row = probe_row; pc.velocity_row = 1;
    pc.npoints = probe_npoints; pc.points = probe_points; pc.grain_extent = 1;
    DIE(lbmdem_probe_enable(h, &pc), "probe_enable");
    g_probe_file = fopen(probe_path, "w");
    if (!g_probe_file) { perror(probe_path); return EXIT_FAILURE; }
    g_probe_handle = h;
    scene.say = say_and_drain;
  }
  if (max_steps < 0 || max_steps > nbsteps)
    DIE(lbmdem_run_scene(h, comm, max_steps < 0 ? LONG_MAX : max_steps - nbsteps, &scene, &done), "run_scene");
  nbsteps += done.steps_done;
  DIE(lbmdem_sync(h), "sync");
  DIE(lbmdem_output_drain(h), "output_drain");   /* (lbmdem_run_scene has drained already: the files are part of the time) */
  if (probe_path) {
    DIE(drain_probes(), "probe_read");
    fclose(g_probe_file);
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  if (ckpt_out) {
    if (comm) DIE(lbmdem_comm_sync_carries(h, comm), "comm_sync_carries");
    if (g_async_ckpt) {   /* the same way as the periodic ones: snapshot, background write with digests, rename */
      DIE(lbmdem_checkpoint_save_async(h, ckpt_out), "checkpoint_save_async");
      DIE(lbmdem_output_drain(h), "output_drain");
    } else if (g_ckpt_every > 0) {   /* FILE holds a periodic checkpoint: replaced only by a complete one */
      char tmp[4200];
      snprintf(tmp, sizeof tmp, "%s.tmp", ckpt_out);
      DIE(lbmdem_checkpoint_save(h, tmp), "checkpoint_save");
      if (rename(tmp, ckpt_out) != 0) { perror(ckpt_out); return EXIT_FAILURE; }
    } else {
      DIE(lbmdem_checkpoint_save(h, ckpt_out), "checkpoint_save");
    }
  }
  long geometry[6] = {0, 0, 0, 0, 0, 0};
  if (g_dump_geometry) {   /* obst_writing (main.c:1601-1641) */
    DIE(lbmdem_write_obst(h, g_dump_geometry), "write_obst");
    if (g_run_stats) DIE(lbmdem_geometry_stats(h, geometry), "geometry_stats");
  }
  long densities[4] = {0, 0, 0, 0};
  if (g_densities) {   /* write_densities (main.c:482-566), numbered like the next frame */
    int nfile = max_steps < 0 || done.steps_done > 0 ? done.nfile : (int)(nbsteps / cfg.phys.stepFilm);
    DIE(lbmdem_write_densities(h, g_densities, nfile), "write_densities");
    DIE(lbmdem_densities_stats(h, densities), "densities_stats");
  }
  double sum = serial_density(h, comm);
  double secs = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
  if (comm) { /* the slowest rank's time */
    double tmax[64] = {0};
    tmax[g_rank] = secs;
    DIE(lbmdem_comm_allreduce_sum(comm, tmax, g_world), "allreduce");
    for (int r = 0; r < g_world; ++r) if (tmax[r] > secs) secs = tmax[r];
  }
  long lbm_steps = g_dry ? 0 : (nbsteps + cfg.npDEM - 1) / cfg.npDEM;
  if (g_rank == 0) {
    fprintf(stderr, "final_density: %f\n", sum);
    if (g_densities) fprintf(stderr, "densities: pressure_bytes %ld velocity_bytes %ld bands %ld\n", densities[0], densities[1], densities[2]);
    fprintf(stderr, "time: %e\n", secs);
    fprintf(stderr, "dem_steps: %ld\n", nbsteps);
    fprintf(stderr, "MLUPS: %.1f  DEM-steps/s: %.1f  (%d GPU%s)\n", 1e-6 * (double)lx * ly * lbm_steps / secs, nbsteps / secs,
            g_world, g_world > 1 ? "s" : "");
    if (g_run_stats) {   /* how the DEM sub-steps were launched (rank 0's handle) */
      long launches = 0, substeps = 0, recoveries = 0, paints = 0;
      DIE(lbmdem_dem_chain_stats(h, &launches, &substeps, NULL, NULL), "dem_chain_stats");
      DIE(lbmdem_dem_chain_recoveries(h, &recoveries), "dem_chain_recoveries");
      DIE(lbmdem_dem_chain_paints(h, &paints), "dem_chain_paints");
      fprintf(stderr, "dem_chain: launches %ld substeps %ld recoveries %ld paints %ld\n", launches, substeps, recoveries, paints);
      if (g_dump_geometry)
        fprintf(stderr, "geometry: solid_nodes %ld active_nodes %ld links %ld links_near %ld links_far %ld solid_slots %ld\n",
                geometry[0], geometry[1], geometry[2], geometry[3], geometry[4], geometry[5]);
      if (g_async_frames) DIE(print_async_stats(h, lbmdem_output_stats, "async_output", "ms_drain"), "output_stats");
      if (g_async_ckpt) DIE(print_async_stats(h, lbmdem_output_stats_checkpoint, "async_checkpoint", "ms_hold"), "output_stats_checkpoint");
      if (g_async_dem) DIE(print_async_stats(h, lbmdem_output_stats_dem, "async_dem", "ms_stats_wait"), "output_stats_dem");
    }
  }
  now = time(NULL);
  SAY("End local time and date: %s", asctime(localtime(&now)));
  lbmdem_comm_destroy(comm);
  lbmdem_destroy(h);
  lbmdem_free_host(r); lbmdem_free_host(x1); lbmdem_free_host(x2);
  return 0;
}
