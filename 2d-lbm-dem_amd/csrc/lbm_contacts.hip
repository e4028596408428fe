// lbm_contacts.hip -- the contact network export (lbmdem_contact_stats, lbmdem_download_contacts, lbmdem_write_contacts,
// lbmdem_set_contacts_output, lbmdem_write_contacts_files; include/lbmdem_hip.h): the reference's `struct contact` (main.c:167-174),
// which it declares and never fills, and the force-chain map write_forces was meant to draw (main.c:469).
//
// The per-contact values of a sub-step exist only in the registers of the sub-step kernels. They are re-derived here, with the
// same device functions (dem_laws.h), from the state the LAST sub-step started from -- the other half of the kinematics ping-pong,
// kin[1 - kcur] -- with that sub-step's pair list, wall flags, law and parameters (lbmdem_handle::contacts_P, kept when it was
// launched). A wall moved by hand since (lbmdem_move_walls) makes the export refuse: the handle's walls are then not the ones of
// the records (lbmdem_handle::walls_moved). Nothing here is on the step path: the kernels only read the handle's state.
//
// Three steps on the handle's stream, the order fixed without atomics:
//   k_contacts_count  one lane per entry of the symmetric list; a workgroup owns CT_GRAINS consecutive grains and therefore a
//                     contiguous slice of the list (as k_dem_entries). Per workgroup the number of pair records and of wall
//                     records, and the six counters of lbmdem_contact_stats;
//   an exclusive scan of the per-workgroup counts, all pair counts first, then all wall counts (hipcub::DeviceScan);
//   k_contacts_emit   the same evaluation once more; a record's slot is the workgroup's base + the records of the rounds and
//                     wavefronts before + the lane's rank in its wavefront's ballot.
// lbmdem_contacts_records is these three steps for whoever wants the records on the device: the download below, and the cluster
// analysis (lbm_clusters.hip), which never copies them to the host.
// Double-precision library only: the other one's entry points refuse. The files' formatter is host code and exists in both.
// Front end, as every export's: whole_handle() and SP_REFUSE() (lbmdem_handle.h) for the refusals, MemPool::grow (lbm_mem.h) for
// the record buffer kept on the handle, OutFile (lbm_outfile.h) for the two files.
#include "lbm_outfile.h"

#include <errno.h>

#ifndef LBMDEM_SINGLE_PRECISION
#include "dem_laws.h"

#include <hipcub/hipcub.hpp>
#endif

namespace {

#ifndef LBMDEM_SINGLE_PRECISION
static_assert(sizeof(lbmdem_contact) == 48, "lbmdem_contact is the record the kernel stores: three 16-byte stores");
static_assert(offsetof(lbmdem_contact, dn) == 8 && offsetof(lbmdem_contact, nx) == 16 && offsetof(lbmdem_contact, fn) == 32,
              "lbmdem_contact's layout");

constexpr int CT_GRAINS = 64;     // grains per workgroup: one per lane of the first wavefront
constexpr int CT_THREADS = 256;   // list entries per round

struct ContactsJob {
  Kin K;                        // the state the sub-step started from
  const real* r;
  const int *offsets, *nbr, *own;
  const unsigned char* wallflags;
  DemParams P;                  // of that sub-step (gate: null)
  int n, nwg;
  long long* counts;            // count: [2 nwg + 1] pair records per workgroup, then wall records per workgroup, then 0 (may be
                                // null); emit: their exclusive scan
  unsigned long long* census;   // [6], count only
  lbmdem_contact* out;          // emit only
  long long cap;                // records `out` holds
};

__device__ __forceinline__ int lanes_below(unsigned long long m) {   // set bits of m below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// did the law take its Coulomb clamp branch (main.c:766, 1386)? Both branches assign a value of another magnitude or sign than
// the unclamped ft, so: iff the law's ft is not the unclamped one, formed once more from the law's own vt.
template <bool FILM>
__device__ __forceinline__ bool coulomb_clamped(const Force3& F, const DemParams& P) {
  if (FILM) { const real ft0 = P.kt * F.vt * P.dt; return F.ft != ft0; }
  const double ft0 = -P.kt * F.vt * P.dt;
  return (double)F.ft != ft0;
}

// a record from registers: {i, j, dn}, {nx, ny}, {fn, ft} -- 16 bytes each; 48 * at is a multiple of 16
__device__ __forceinline__ void store_contact(lbmdem_contact* out, long long at, int i, int j, double dn, double nx, double ny,
                                              double fn, double ft) {
  const long long d = __double_as_longlong(dn);
  int4 a;
  a.x = i; a.y = j; a.z = (int)(unsigned)((unsigned long long)d & 0xFFFFFFFFull); a.w = (int)(unsigned)((unsigned long long)d >> 32);
  double2 b, c;
  b.x = nx; b.y = ny;
  c.x = fn; c.y = ft;
  char* p = reinterpret_cast<char*>(out + at);
  *reinterpret_cast<int4*>(p) = a;
  *reinterpret_cast<double2*>(p + 16) = b;
  *reinterpret_cast<double2*>(p + 32) = c;
}

// EMIT = false: counts[] and the census. EMIT = true: the records at the scanned offsets.
template <bool FILM, bool EMIT>
__device__ __forceinline__ void contacts_tile(const ContactsJob& J) {
  __shared__ int sW[4];                    // pair records of each wavefront in this round
  __shared__ int sC[4][4];                 // the wavefronts' pair counters
  __shared__ unsigned char sHas[CT_GRAINS];   // grain of the tile with at least one record
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int g0 = b * CT_GRAINS;
  const int g1 = g0 + CT_GRAINS < J.n ? g0 + CT_GRAINS : J.n;
  const int e0 = J.offsets[g0], e1 = J.offsets[g1];
  if (!EMIT) {
    if (tid < CT_GRAINS) sHas[tid] = 0;
    __syncthreads();
  }
  const long long base = EMIT ? J.counts[b] : 0;
  int npairs = 0;                          // pair records of the rounds before (the same in every lane)
  int c_cand = 0, c_touch = 0, c_clamp = 0, c_fn0 = 0;   // this wavefront's
  for (int start = e0; start < e1; start += CT_THREADS) {   // (every lane stays in the loop: ballots and barriers)
    const int e = start + tid;
    bool cand = false, rec = false, clamp = false, fn0 = false;
    int gi = 0, gj = 0;
    Force3 F = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    if (e < e1) {
      gi = J.own[e]; gj = J.nbr[e];
      cand = gi < gj;   // main.c:1443-1445: the reference evaluates the pair there, once
      // the counting pass looks at the entries of the upper grain too: a grain has a record if any of ITS entries touches
      if (cand || !EMIT) {
        const GrainState a = advance(J.K, J.r, gi, J.P), o = advance(J.K, J.r, gj, J.P);
        bool touched;
        F = contact<FILM>(cand ? a : o, cand ? o : a, J.P, touched);
        rec = cand && touched;
        if (!EMIT) {
          if (touched) sHas[gi - g0] = 1;   // (every writer stores the same byte)
          clamp = rec && coulomb_clamped<FILM>(F, J.P);
          fn0 = rec && F.fn == 0;
        }
      }
    }
    const unsigned long long m = __ballot(rec);
    if (lane == 0) sW[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = sW[w];
      if (w < wave) before += c;
      total += c;
    }
    if (EMIT && rec) {
      const long long at = base + npairs + before + lanes_below(m);
      if (at < J.cap) store_contact(J.out, at, gi, gj, F.dn, F.xn, F.yn, F.fn, F.ft);
    }
    npairs += total;
    if (!EMIT) {
      c_cand += __popcll(__ballot(cand)); c_touch += __popcll(m);
      c_clamp += __popcll(__ballot(clamp)); c_fn0 += __popcll(__ballot(fn0));
    }
    __syncthreads();   // sW is written again in the next round
  }
  if (!EMIT && lane == 0) { sC[wave][0] = c_cand; sC[wave][1] = c_touch; sC[wave][2] = c_clamp; sC[wave][3] = c_fn0; }
  // the walls of the tile's grains: bottom, top, left, right (main.c:1455-1508), one grain per lane of the first wavefront
  if (wave == 0) {
    const int i = g0 + lane;
    const bool have = i < g1;
    WallForce WB = {0., 0., 0., 0., 0., 0.}, WT = WB, WL = WB, WR = WB;
    bool hB = false, hT = false, hL = false, hR = false;
    if (have) {
      const GrainState me = advance(J.K, J.r, i, J.P);
      const unsigned wf = J.wallflags[i];
      if (wf & 1u) { WB = wall_bottom(me, J.P); hB = WB.dn < 0; }
      if (wf & 2u) { WT = wall_top(me, J.P); hT = WT.dn < 0; }
      if (wf & 4u) { WL = wall_left(me, J.P); hL = WL.dn < 0; }
      if (wf & 8u) { WR = wall_right(me, J.P); hR = WR.dn < 0; }
    }
    const unsigned long long mB = __ballot(hB), mT = __ballot(hT), mL = __ballot(hL), mR = __ballot(hR);
    const int nwall = __popcll(mB) + __popcll(mT) + __popcll(mL) + __popcll(mR);
    if (EMIT) {
      // the records of the lower grains of the tile, then this grain's own in the order B, T, L, R
      long long at = J.counts[J.nwg + b] + lanes_below(mB) + lanes_below(mT) + lanes_below(mL) + lanes_below(mR);
      if (hB) { if (at < J.cap) store_contact(J.out, at, i, LBMDEM_WALL_B, WB.dn, 0., 1., WB.fn, WB.ft); ++at; }
      if (hT) { if (at < J.cap) store_contact(J.out, at, i, LBMDEM_WALL_T, WT.dn, 0., -1., WT.fn, WT.ft); ++at; }
      if (hL) { if (at < J.cap) store_contact(J.out, at, i, LBMDEM_WALL_L, WL.dn, 1., 0., WL.fn, WL.ft); ++at; }
      if (hR) { if (at < J.cap) store_contact(J.out, at, i, LBMDEM_WALL_R, WR.dn, -1., 0., WR.fn, WR.ft); ++at; }
    } else {
      // (the pair rounds' stores to sHas are behind the loop's last barrier, or there was no round)
      const bool any = have && (sHas[lane] != 0 || hB || hT || hL || hR);
      const int ngrains = __popcll(__ballot(any));
      if (lane == 0) {
        if (J.counts) { J.counts[b] = npairs; J.counts[J.nwg + b] = nwall; }
        if (nwall) atomicAdd(&J.census[4], (unsigned long long)nwall);
        if (ngrains) atomicAdd(&J.census[5], (unsigned long long)ngrains);
      }
    }
  }
  if (!EMIT) {
    __syncthreads();
    if (tid < 4) {
      const int s = sC[0][tid] + sC[1][tid] + sC[2][tid] + sC[3][tid];
      if (s) atomicAdd(&J.census[tid], (unsigned long long)s);
    }
  }
}

template <bool FILM>
__global__ __launch_bounds__(CT_THREADS) void k_contacts_count(const ContactsJob J) { contacts_tile<FILM, false>(J); }
template <bool FILM>
__global__ __launch_bounds__(CT_THREADS) void k_contacts_emit(const ContactsJob J) { contacts_tile<FILM, true>(J); }

// what the export describes: the last sub-step, when it was a table sub-step
int contacts_job(lbmdem_handle* h, const char* who, ContactsJob* J) {
  RC_TRY(whole_handle(h, who));
  if (!h->contacts_valid || !h->verlet_ok)
    return fail(LBMDEM_EINVAL, "%s: the last sub-step was no table sub-step, or the state it started from has been replaced since "
                               "(lbmdem_set_diagnostics(h, 1), or the sub-step that reaches a multiple of 4000)", who);
  if (h->contacts_walls != h->walls_moved)
    return fail(LBMDEM_EINVAL, "%s: a wall has been moved since the last table sub-step (lbmdem_move_walls): its records belong to "
                               "walls the handle no longer has, and the next table sub-step (lbmdem_set_diagnostics(h, 1)) makes "
                               "new ones", who);
  if (*h->ovf_host) return fail(LBMDEM_ENOMEM, "Verlet list overflow (more than %ld symmetric entries)", h->V.cap);
  *J = ContactsJob{};
  J->K = h->kin[1 - h->kcur];
  J->r = h->r;
  J->offsets = h->V.offsets; J->nbr = h->V.nbr; J->own = h->V.own;
  J->wallflags = h->V.wallflags;
  J->P = h->contacts_P;
  J->P.gate = nullptr;
  J->P.vib = nullptr;
  J->n = h->n;
  J->nwg = (h->n + CT_GRAINS - 1) / CT_GRAINS;
  return LBMDEM_OK;
}

// the staging that does not depend on the record count, once per handle
int contacts_stage(lbmdem_handle* h, int nwg) {
  auto& X = h->cx;
  if (X.nwg == nwg) return LBMDEM_OK;
  const int items = 2 * nwg + 1;
  HIP_TRY(h->mem.dev(&X.census, 6));
  HIP_TRY(h->mem.dev(&X.counts, (size_t)items));
  HIP_TRY(h->mem.dev(&X.offsets, (size_t)items));
  size_t bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, X.counts, X.offsets, items, h->stream));
  HIP_TRY(h->mem.dev(&X.scan_tmp, bytes));
  X.scan_bytes = bytes;
  X.nwg = nwg;
  return LBMDEM_OK;
}

// pass 1: J.counts (may be null) and the census
int contacts_count(lbmdem_handle* h, const ContactsJob& J) {
  HIP_TRY(hipMemsetAsync(J.census, 0, 6 * sizeof(unsigned long long), h->stream));
  if (h->contacts_film) hipLaunchKernelGGL(k_contacts_count<true>, dim3(J.nwg), dim3(CT_THREADS), 0, h->stream, J);
  else hipLaunchKernelGGL(k_contacts_count<false>, dim3(J.nwg), dim3(CT_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}
#endif   // !LBMDEM_SINGLE_PRECISION

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

// the header of the force map and one filled disc per grain (main.c:449-460), fm the grey level: DEM%06d.ps (lbmdem_output.hip)
// and the contact network's map below start with it. Every array is read at i * stride.
void lbmdem_ps_head(FILE* fp, int n, const double* x1, const double* x2, const double* r, const double* fm, size_t stride, int lx,
                    int ly) {
  const double margin = 10 * r[0], hrx1 = lx, hry2 = ly;  // main.c:449
  fprintf(fp, "%%!PS-Adobe-3.0 EPSF-3.0 \n");
  fprintf(fp, "%%%%BoundingBox: %f %f %f %f \n", -margin, -margin, hrx1 + margin, hry2 + margin);
  fprintf(fp, "%%%%Creator: lbmdem-hip \n");
  fprintf(fp, "%%%%Title: DEM Grains & Forces \n");
  fprintf(fp, "0.1 setlinewidth 0.0 setgray \n");
  for (int i = 0; i < n; i++)
    fprintf(fp, "newpath %le %le %le 0.0 setlinewidth %.2f setgray 0 360 arc gsave fill grestore\n", x1[i * stride] * 10000,
            x2[i * stride] * 10000, r[i * stride] * 10000, (0.8 - fm[i * stride] / 2));
}

int lbmdem_write_contacts_files(const char* dir, int nfile, int n, const double* r, const double* x1, const double* x2,
                                const double* fm, const lbmdem_contact* c, long count, int lx, int ly) {
  if (n < 1 || !r || !x1 || !x2 || !fm || count < 0 || (count > 0 && !c)) return fail(LBMDEM_EINVAL, "bad lbmdem_write_contacts_files arguments");
  for (long k = 0; k < count; ++k) {
    const bool wall = c[k].j <= LBMDEM_WALL_B && c[k].j >= LBMDEM_WALL_R;
    if (c[k].i < 0 || c[k].i >= n || (!wall && (c[k].j < 0 || c[k].j >= n)))
      return fail(LBMDEM_EINVAL, "lbmdem_write_contacts_files: record %ld names a grain outside [0, %d) or an unknown wall", k, n);
  }
  OutFile F;
  RC_TRY(F.open("w", dir, "contacts%.6i.dat", nfile));
  FILE* fp = F.fp;
  fprintf(fp, "# i j dn nx ny fn ft\n");
  for (long k = 0; k < count; ++k)
    fprintf(fp, "%d %d %le %le %le %le %le\n", c[k].i, c[k].j, c[k].dn, c[k].nx, c[k].ny, c[k].fn, c[k].ft);
  RC_TRY(F.close());
  RC_TRY(F.open("w", dir, "DEM%.6i_chains.ps", nfile));
  fp = F.fp;
  lbmdem_ps_head(fp, n, x1, x2, r, fm, 1, lx, ly);
  for (long k = 0; k < count; ++k) {
    if (c[k].j < 0 || !(c[k].fn > 0)) continue;   // walls have no second centre; a line of width 0 is no chain
    const int i = c[k].i, j = c[k].j;
    fprintf(fp, "%le setlinewidth \n 0.0 setgray \n", c[k].fn);   // main.c:469, with the term it comments out
    fprintf(fp, "1 setlinecap \n newpath \n");
    fprintf(fp, "%le %le moveto \n %le %le lineto\n", x1[i] * 10000, x2[i] * 10000, x1[j] * 10000, x2[j] * 10000);
    fprintf(fp, "stroke \n");
  }
  return F.close();
}

#ifdef LBMDEM_SINGLE_PRECISION
int lbmdem_contact_stats(lbmdem_handle* h, long*) { SP_REFUSE(h, "the contact network export"); }
int lbmdem_download_contacts(lbmdem_handle* h, lbmdem_contact*, long, long*) { SP_REFUSE(h, "the contact network export"); }
int lbmdem_write_contacts(lbmdem_handle* h, const char*, int) { SP_REFUSE(h, "the contact network export"); }
int lbmdem_set_contacts_output(lbmdem_handle* h, int) { SP_REFUSE(h, "the contact network export"); }
#else

// count, scan, total and -- when the records fit into `room` -- emit: the records of the last table sub-step in h->cx.rec, on the
// device, the *npairs pair records first (lbmdem_download_contacts, and lbm_clusters.hip with room = LONG_MAX). Synchronises once,
// for the total; the emit is left on the stream.
int lbmdem_contacts_records(lbmdem_handle* h, const char* who, long room, long* npairs, long* total) {
  ContactsJob J;
  RC_TRY(contacts_job(h, who, &J));
  RC_TRY(contacts_stage(h, J.nwg));
  auto& X = h->cx;
  const int items = 2 * J.nwg + 1;
  J.census = X.census;
  J.counts = X.counts;
  // (the item behind the last workgroup is an empty one: its offset is the number of records)
  HIP_TRY(hipMemsetAsync(X.counts + items - 1, 0, sizeof(long long), h->stream));
  RC_TRY(contacts_count(h, J));
  size_t bytes = X.scan_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(X.scan_tmp, bytes, X.counts, X.offsets, items, h->stream));
  long long ends[2] = {0, 0};   // the offset of the first wall record, and of the item behind the last
  HIP_TRY(hipMemcpyAsync(&ends[0], X.offsets + J.nwg, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&ends[1], X.offsets + items - 1, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *npairs = (long)ends[0];
  *total = (long)ends[1];
  if (ends[1] == 0 || room < ends[1]) return LBMDEM_OK;
  // grown with some room: the count moves a little from table to table
  if (X.rec_cap < ends[1]) HIP_TRY(h->mem.grow(&X.rec, &X.rec_cap, (long)(ends[1] + ends[1] / 8 + 64)));
  J.counts = X.offsets;
  J.out = X.rec;
  J.cap = ends[1];
  if (h->contacts_film) hipLaunchKernelGGL(k_contacts_emit<true>, dim3(J.nwg), dim3(CT_THREADS), 0, h->stream, J);
  else hipLaunchKernelGGL(k_contacts_emit<false>, dim3(J.nwg), dim3(CT_THREADS), 0, h->stream, J);
  HIP_TRY(hipGetLastError());
  return LBMDEM_OK;
}

int lbmdem_contact_stats(lbmdem_handle* h, long* counts6) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!counts6) return fail(LBMDEM_EINVAL, "null buffer");
  ContactsJob J;
  RC_TRY(contacts_job(h, "lbmdem_contact_stats", &J));
  RC_TRY(contacts_stage(h, J.nwg));
  J.census = h->cx.census;
  RC_TRY(contacts_count(h, J));
  unsigned long long c[6];
  HIP_TRY(hipMemcpyAsync(c, J.census, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 6; ++k) counts6[k] = (long)c[k];
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {   // (CHECK_H may replay logged runs)
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_download_contacts(lbmdem_handle* h, lbmdem_contact* out, long cap, long* count) try {
  CHECK_H(h);
  CHECK_NOT_SPLIT(h);
  if (!count || (cap > 0 && !out) || cap < 0) return fail(LBMDEM_EINVAL, "null buffer");
  long npairs = 0, total = 0;
  RC_TRY(lbmdem_contacts_records(h, "lbmdem_download_contacts", cap, &npairs, &total));
  *count = total;
  if (cap == 0) return LBMDEM_OK;   // (how many there are)
  if (cap < total) return fail(LBMDEM_EINVAL, "lbmdem_download_contacts: there are %ld records, the buffer holds %ld", total, cap);
  if (total == 0) return LBMDEM_OK;
  HIP_TRY(hipMemcpyAsync(out, h->cx.rec, sizeof(lbmdem_contact) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LBMDEM_OK;
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_write_contacts(lbmdem_handle* h, const char* dir, int nfile) try {
  CHECK_H(h);
  const int n = h->n;
  long count = 0;
  RC_TRY(lbmdem_download_contacts(h, nullptr, 0, &count));
  std::vector<lbmdem_contact> rec((size_t)(count > 0 ? count : 1));
  if (count > 0) RC_TRY(lbmdem_download_contacts(h, rec.data(), count, &count));
  std::vector<double> t(30 * (size_t)n), col(4 * (size_t)n);
  RC_TRY(lbmdem_download_grain_table(h, t.data()));
  double *r = col.data(), *x1 = r + n, *x2 = x1 + n, *fm = x2 + n;
  for (int i = 0; i < n; ++i) {
    const double* o = &t[(size_t)i * 30];
    r[i] = o[9]; x1[i] = o[0]; x2[i] = o[1]; fm[i] = o[18];
  }
  return lbmdem_write_contacts_files(dir, nfile, n, r, x1, x2, fm, rec.data(), count, h->cfg.lx, h->cfg.ly);
} catch (const std::bad_alloc&) {
  return fail(LBMDEM_ENOMEM, "host memory allocation failed");
}

int lbmdem_set_contacts_output(lbmdem_handle* h, int on) {
  if (!h) return fail(LBMDEM_EINVAL, "null handle");
  if (on) RC_TRY(whole_handle(h, "lbmdem_set_contacts_output"));
  h->contacts_output = on != 0;
  return LBMDEM_OK;
}
#endif   // LBMDEM_SINGLE_PRECISION

}  // extern "C"
#pragma GCC visibility pop
