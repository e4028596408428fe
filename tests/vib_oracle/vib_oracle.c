/*
 * vib_oracle.c -- TEST INFRASTRUCTURE: the CPU oracle (oracle/lbmdem_oracle.c, included unchanged) with the reference's
 * shaken box, `vib = 1`. Read against the reference's src/main.c:1699-1706: when vib is set, renderScene first advances
 * the clock t by one DEM time step dt, then adds amp times the sine of freq times the NEW t to the left wall Mgx and,
 * separately (the same product evaluated a second time), to the right wall Mdx -- in the reference's `real`, before the
 * fluid step, the Verlet rebuild and the DEM sub-step, which all read the moved walls (the line about Mby there is
 * commented out). The oracle keeps those walls in s->t, s->Mgx, s->Mdx and reads them in every routine that matters;
 * this file puts that update (vib_move) in front of the oracle's renderScene and of its DEM-only body, plus a getter.
 * Build with the oracle's pinned flags (-O2 -ffp-contract=off: tests/vib_oracle/Makefile).
 */
#include "../../oracle/lbmdem_oracle.c"

static void vib_move(ora_sim* s) {   /* main.c:1700-1705 */
  s->t = s->t + s->dt;
  s->Mgx = s->Mgx + s->amp * sin(s->freq * s->t);
  s->Mdx = s->Mdx + s->amp * sin(s->freq * s->t);
}

ORA_API void vib_render_scene(ora_sim* s) { vib_move(s); ora_render_scene(s); }
ORA_API void vib_steps(ora_sim* s, long n) { for (long k = 0; k < n; ++k) vib_render_scene(s); }
/* the reference without _FLUIDE_ (main.c:16,1709-1719), vibrating: ora_steps_dry's body after the move */
ORA_API void vib_steps_dry(ora_sim* s, long n) {
  for (long k = 0; k < n; ++k) {
    vib_move(s);
    if (s->nbsteps % s->updateVerlet == 0) ora_verlet_rebuild(s);
    ora_dem_substep(s);
  }
}
/* t, Mgx, Mdx, Mby, Mhy */
ORA_API void vib_get_walls(const ora_sim* s, double* out5) {
  out5[0] = s->t; out5[1] = s->Mgx; out5[2] = s->Mdx; out5[3] = s->Mby; out5[4] = s->Mhy;
}
