// lbmdem_scene.hip -- the reference's main loop over the C ABI: `do { renderScene(); ... } while (nbsteps * dt <= duration)`
// (main.c:1879-1890) with everything renderScene hangs on the step counter besides the step itself -- check_density's
// console line (main.c:1715), write_vtk (main.c:1767-1772), write_DEM / write_forces (main.c:1773-1776), the "steps" line
// (main.c:1884-1889). The cadences live in ONE place, the Cadence struct below: lbmdem_scene_schedule lists the events,
// lbmdem_run_scene walks the same list and hands the sub-steps between two events to the run loop in one piece. A handle with
// lbmdem_set_checkpoint_every has one more stop that is no event of the schedule: the step counters that are multiples of its
// cadence, where the loop saves a checkpoint behind whatever else that sub-step brings.

#include "lbm_outfile.h"

#include <limits.h>
#include <time.h>

namespace {

constexpr long STEP_CONSOLE = 400;   // main.c:140
constexpr long STEP_STROB = 4000;    // main.c:142

// first s' >= 1 with (double)s' * dt > duration -- the predicate the loop evaluates (main.c:1890), not a division: a
// candidate from the quotient is moved until the predicate flips. LONG_MAX: never.
long first_stop_step(double dt, double duration) {
  if (duration < 0.) return LONG_MAX;
  auto over = [&](long s) { return (double)s * dt > duration; };
  const double q = duration / dt;
  if (!(q < 4.0e18)) return LONG_MAX;
  long s = (long)q;
  if (s < 1) s = 1;
  while (s > 1 && over(s - 1)) --s;
  while (!over(s)) ++s;
  return s;
}

struct Cadence {
  long npDEM, film, verlet, stop;
  int fluid;
  // `s`: the step counter BEFORE a sub-step, s + 1 after it
  bool console(long s) const { return fluid && s % npDEM == 0 && s % STEP_CONSOLE == 0; }   // main.c:1710,1715
  bool vtk(long s) const { return (s + 1) % film == 0; }                                    // main.c:1767
  bool dem(long s) const { return (s + 1) % STEP_STROB == 0; }                              // main.c:1773
  bool line(long s) const { return (s + 1) % verlet == 0; }                                 // main.c:1884
  bool stops(long s) const { return s + 1 >= stop; }                                        // main.c:1890
  // the first sub-step in [s, end) that has an event; `end` when there is none
  long next(long s, long end) const {
    auto up = [](long v, long m) { return (v + m - 1) / m * m; };   // smallest multiple of m that is >= v
    long e = end;
    auto take = [&](long c) { if (c < e) e = c; };
    if (fluid) { long c = up(s, STEP_CONSOLE); while (c < e && c % npDEM != 0) c += STEP_CONSOLE; take(c); }
    take(up(s + 1, film) - 1);
    take(up(s + 1, STEP_STROB) - 1);
    take(up(s + 1, verlet) - 1);
    if (stop != LONG_MAX) take(stop - 1 > s ? stop - 1 : s);
    return e;
  }
  // the events of sub-step s in the loop's order; nfile is the frame counter before it and is advanced; -> how many
  int events(long s, int* nfile, lbmdem_scene_event ev[5]) const {
    int k = 0;
    if (console(s)) ev[k++] = lbmdem_scene_event{LBMDEM_SCENE_CONSOLE_DENSITY, *nfile, s};
    if (vtk(s)) { ev[k++] = lbmdem_scene_event{LBMDEM_SCENE_VTK, *nfile, s + 1}; ++*nfile; }
    if (dem(s)) ev[k++] = lbmdem_scene_event{LBMDEM_SCENE_DEM, *nfile, s + 1};
    if (line(s)) ev[k++] = lbmdem_scene_event{LBMDEM_SCENE_STEPS_LINE, *nfile, s + 1};
    if (stops(s)) ev[k++] = lbmdem_scene_event{LBMDEM_SCENE_STOP, *nfile, s + 1};
    return k;
  }
};

int cadence_of(const lbmdem_config* cfg, long nbsteps0, double duration, int fluid, Cadence* out) {
  if (!cfg || nbsteps0 < 0) return fail(LBMDEM_EINVAL, "bad argument");
  if (cfg->npDEM < 1 || cfg->phys.updateVerlet < 1 || cfg->phys.stepFilm < 1) return fail(LBMDEM_EINVAL, "npDEM, updateVerlet, stepFilm must be >= 1");
  if (!(cfg->dt > 0.)) return fail(LBMDEM_EINVAL, "dt must be > 0");
  *out = Cadence{cfg->npDEM, cfg->phys.stepFilm, cfg->phys.updateVerlet, first_stop_step(cfg->dt, duration), fluid ? 1 : 0};
  return LBMDEM_OK;
}

struct Speaker {
  const lbmdem_scene* sc;
  bool on;   // rank 0
  void operator()(const char* line) const {
    if (!on) return;
    if (sc->say) sc->say(sc->user, line);
    else fputs(line, stdout);
  }
};

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int lbmdem_scene_schedule(const lbmdem_config* cfg, long nbsteps0, long n, double duration, int fluid,
                          lbmdem_scene_event* out, long cap, long* count) {
  Cadence cad;
  RC_TRY(cadence_of(cfg, nbsteps0, duration, fluid, &cad));
  if (n < 0 || cap < 0 || (cap > 0 && !out) || !count || nbsteps0 > LONG_MAX - n) return fail(LBMDEM_EINVAL, "bad argument");
  const long end = nbsteps0 + n;
  int nfile = (int)(nbsteps0 / cad.film);   // main.c:147
  long total = 0;
  for (long s = cad.next(nbsteps0, end); s < end; s = cad.next(s + 1, end)) {
    lbmdem_scene_event ev[5];
    const int k = cad.events(s, &nfile, ev);
    for (int j = 0; j < k; ++j, ++total) if (total < cap) out[total] = ev[j];
    if (cad.stops(s)) break;
  }
  *count = total;
  return LBMDEM_OK;
}

// lbmdem_set_flow_output: one line of <dir>/flow.data -- nbsteps * dt and the eight numbers of lbmdem_flow_sums -- behind a header
// line when the file is new
static int flow_data_line(lbmdem_handle* h, const char* dir) {
  double s[8];
  RC_TRY(lbmdem_flow_sums(h, s));
  OutFile F;
  RC_TRY(F.open("a", dir, "flow.data"));
  FILE* fp = F.fp;
  if (fseek(fp, 0, SEEK_END) == 0 && ftell(fp) == 0) fprintf(fp, "# t n_fluid sum_rho sum_ke sum_diss sum_enstrophy max_u2 max_gdot max_abs_div\n");
  fprintf(fp, "%le", h->nbsteps * h->cfg.dt);
  for (int k = 0; k < 8; ++k) fprintf(fp, " %le", s[k]);
  fprintf(fp, "\n");
  return F.close();
}

static int run_scene_loop(lbmdem_handle* h, lbmdem_comm* comm, long n, const lbmdem_scene* sc, lbmdem_scene_result* res) {
  CHECK_H(h);
  if (!sc || n < 0) return fail(LBMDEM_EINVAL, "bad argument");
  if (comm && !sc->fluid) return fail(LBMDEM_EINVAL, "a run without the fluid is a single-domain run (the strips exist for the fluid)");
  int rank = 0, world = 1;
  if (comm) RC_TRY(lbmdem_comm_rank_world(comm, &rank, &world));
  const lbmdem_config& cfg = h->cfg;
  const long first = h->nbsteps;
  Cadence cad;
  RC_TRY(cadence_of(&cfg, first, sc->duration, sc->fluid, &cad));
  const long end = n > LONG_MAX - first ? LONG_MAX : first + n;
  const char* dir = sc->dir;
  const Speaker say{sc, rank == 0};
  int nfile = (int)(first / cad.film);   // main.c:147
  int stopped = 0;
  double density = 0.;
  char text[1024];
  auto stretch = [&](long k) -> int {   // k x renderScene's step, in one call of the run loop
    if (k <= 0) return LBMDEM_OK;
    if (comm) return lbmdem_comm_run(h, comm, k);
    return sc->fluid ? lbmdem_run(h, k) : lbmdem_run_dem(h, k);
  };
  const long ck = comm ? 0 : h->ckpt_every;   // lbmdem_set_checkpoint_every: single-domain runs
  const bool mean_out = dir && sc->fluid && !comm && h->mean_output_mask != 0;   // lbmdem_set_mean_output
  {   // a window that has just come out of a checkpoint goes on where it was when it is the window this call would open
    const bool resume = mean_out && h->mean.on && h->mean.resumed && h->mean.mask == h->mean_output_mask &&
                        h->mean.every == h->mean_output_every;
    h->mean.resumed = false;   // (one shot, whatever this call does)
    if (mean_out && !resume) RC_TRY(lbmdem_mean_begin(h, h->mean_output_mask, h->mean_output_every));
  }
  for (long s = first; s < end && !stopped;) {
    long e = cad.next(s, end);
    if (ck > 0) {   // the sub-step that brings the counter to the next multiple of the cadence ends a stretch as well
      const long c = (s + ck) / ck * ck - 1;
      if (c < e) e = c;
    }
    if (e >= end) { RC_TRY(stretch(end - s)); break; }
    if (cad.console(e)) {
      // check_density is printed between the fluid step of sub-step e and the rest of it (main.c:1710-1718): the phases
      // one by one
      RC_TRY(stretch(e - s));
      if (lbmdem_vibration(h) == 1) RC_TRY(lbmdem_move_walls(h));   // main.c:1700-1705
      if (comm) RC_TRY(lbmdem_comm_lbm_step(h, comm)); else RC_TRY(lbmdem_lbm_step(h));
      // ONE serial chain over the whole lattice (main.c:1249-1260): with strips it runs through the ranks in x order, rank r
      // continues from rank r - 1's sum (handed on through the all-reduce: everybody else contributes 0)
      double sum = 0.;
      for (int r = 0; r < world; ++r) {
        double v = 0.;
        if (r == rank) RC_TRY(lbmdem_total_density_serial(h, sum, &v, nullptr));
        if (comm) RC_TRY(lbmdem_comm_allreduce_sum(comm, &v, 1));
        sum = v;
      }
      density = sum;
      snprintf(text, sizeof text, "Iteration Number %ld, Total density in the system %f\n", e, sum);   // main.c:1259
      say(text);
      if (e % cad.verlet == 0) RC_TRY(lbmdem_verlet_rebuild(h));   // main.c:1721-1724
      RC_TRY(lbmdem_dem_substep(h));                               // main.c:1733-1764
    } else {
      RC_TRY(stretch(e + 1 - s));   // the events of sub-step e all follow it
    }
    s = e + 1;
    if (cad.vtk(e)) {   // write_vtk sits inside `#ifdef _FLUIDE_` (main.c:1768-1770); nFile++ does not
      if (dir && sc->fluid) { if (comm) RC_TRY(lbmdem_comm_write_vtk(h, comm, dir, nfile)); else if (async_frames_on(h)) RC_TRY(lbmdem_write_vtk_async(h, dir, nfile)); else RC_TRY(lbmdem_write_vtk(h, dir, nfile)); }
      if (dir && sc->fluid && !comm && h->flow_output) RC_TRY(lbmdem_write_flow(h, dir, nfile));   // lbmdem_set_flow_output
      if (dir && sc->fluid && !comm && h->tracer_output) RC_TRY(lbmdem_write_tracers(h, dir, nfile));   // lbmdem_set_tracer_output
      if (dir && sc->fluid && !comm && h->scalar_output && h->scalar.on) RC_TRY(lbmdem_write_scalar(h, dir, nfile));   // lbmdem_set_scalar_output
      if (mean_out && h->mean.samples > 0) {   // (the writers above have settled the handle: the count is that of the samples made)
        RC_TRY(lbmdem_write_mean(h, dir, nfile));
        RC_TRY(lbmdem_mean_reset(h));
      }
      nfile++;
    }
    // (with strips the sub-step before was run by rank 0 on a full replica, lbmdem_comm_run: it holds the whole table)
    if (cad.dem(e) && dir && rank == 0) {
      if (!comm && async_dem_on(h)) {
        RC_TRY(lbmdem_write_dem_async(h, dir, nfile, 1, h->scene_energies));   // the energies now, the files behind the run's back
      } else {
        RC_TRY(lbmdem_write_dem(h, dir, nfile, h->scene_energies));
        RC_TRY(lbmdem_write_forces(h, dir, nfile));
      }
      if (!comm && h->contacts_output) RC_TRY(lbmdem_write_contacts(h, dir, nfile));   // lbmdem_set_contacts_output
      if (!comm && h->clusters_output) RC_TRY(lbmdem_write_clusters(h, dir, nfile, h->clusters_fmin, h->clusters_relative, h->clusters_zmin));   // lbmdem_set_clusters_output
      if (!comm && h->structure_output) RC_TRY(lbmdem_write_structure(h, dir, nfile, h->structure_rcut, h->structure_nbins, h->structure_shell));   // lbmdem_set_structure_output
      if (!comm && h->voronoi_output) RC_TRY(lbmdem_write_voronoi(h, dir, nfile, h->voronoi_rcut));   // lbmdem_set_voronoi_output
      if (!comm && h->strain_output) RC_TRY(lbmdem_write_strain(h, dir, nfile, h->strain_rcut, h->strain_incremental));   // lbmdem_set_strain_output
      if (!comm && h->pores_output) RC_TRY(lbmdem_write_pores(h, dir, nfile, h->pores_conn, h->pores_plane));   // lbmdem_set_pores_output
      if (!comm && h->clearance_output) RC_TRY(lbmdem_write_clearance(h, dir, nfile, h->clearance_plane));   // lbmdem_set_clearance_output
      if (!comm && h->network_output) RC_TRY(lbmdem_write_network(h, dir, nfile, h->network_merge, h->network_plane));   // lbmdem_set_network_output
      if (!comm && h->netflux_output) RC_TRY(lbmdem_write_netflux(h, dir, nfile, h->netflux_merge, h->netflux_level));   // lbmdem_set_netflux_output
      if (!comm && h->netsolve_output) RC_TRY(lbmdem_write_netsolve(h, dir, nfile, h->netsolve_merge, h->netsolve_level, h->netsolve_from, h->netsolve_band, h->netsolve_to, h->netsolve_rtol, h->netsolve_max_iter));   // lbmdem_set_netsolve_output
      if (!comm && h->drainage_output) RC_TRY(lbmdem_write_drainage(h, dir, nfile, h->drainage_from, h->drainage_band, h->drainage_to, h->drainage_plane));   // lbmdem_set_drainage_output
      if (!comm && h->geodesic_output) RC_TRY(lbmdem_write_geodesic(h, dir, nfile, h->geodesic_from, h->geodesic_band, h->geodesic_to, h->geodesic_conn, h->geodesic_min_d2, h->geodesic_plane));   // lbmdem_set_geodesic_output
      if (!comm && h->coarse_cw > 0) RC_TRY(lbmdem_write_coarse(h, dir, nfile, h->coarse_cw, h->coarse_ch));   // lbmdem_set_coarse_output
      if (!comm && h->flow_output) RC_TRY(flow_data_line(h, dir));   // lbmdem_set_flow_output
      if (!comm && h->scalar_output && h->scalar.on) RC_TRY(lbmdem_scalar_data_line(h, dir));   // lbmdem_set_scalar_output
    }
    if (cad.line(e)) {   // main.c:1884-1889
      const double* E = h->scene_energies;
      time_t now = time(NULL);
      snprintf(text, sizeof text, "steps %li steps %le KE %le PE %le SE %le WF %le INCE %le SLIP %le RW %le Time %s \n", s,
               s * cfg.dt, E[0], E[1], E[2], E[4], E[5], E[6], E[7], asctime(localtime(&now)));
      say(text);
    }
    if (ck > 0 && s % ck == 0) {   // behind the sub-step's other events; in the background where slots exist
      if (async_ckpt_on(h)) RC_TRY(lbmdem_checkpoint_save_async(h, h->ckpt_path));
      else RC_TRY(lbmdem_ckpt_save_replacing(h, h->ckpt_path));
    }
    if (cad.stops(e)) stopped = 1;   // main.c:1890
  }
  if (res) {
    res->steps_done = h->nbsteps - first;
    res->nfile = nfile;
    res->stopped = stopped;
    for (int k = 0; k < 8; ++k) res->energies8[k] = h->scene_energies[k];
    res->last_density = density;
  }
  return LBMDEM_OK;
}

// With frames, tables or checkpoints in the background (lbmdem_set_async_output, lbmdem_set_async_dem,
// lbmdem_set_async_checkpoint) the loop's VTK and DEM events and its cadence checkpoints are only queued: the files of the schedule exist when the call returns, so it drains first -- also when the loop ends early with an error, which is then the one
// returned; otherwise a failure of the writer is.
int lbmdem_run_scene(lbmdem_handle* h, lbmdem_comm* comm, long n, const lbmdem_scene* sc, lbmdem_scene_result* res) {
  const int rc = run_scene_loop(h, comm, n, sc, res);
  if (!h || !h->aout) return rc;
  if (rc != LBMDEM_OK) {   // keep the loop's error text: wait here, leave the writer's report to the next call
    lbmdem_async_wait_idle(h);
    return rc;
  }
  return lbmdem_output_drain(h);
}

}  // extern "C"
#pragma GCC visibility pop
