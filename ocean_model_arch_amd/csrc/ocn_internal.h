// ocn_internal.h -- shared internals of libocn_sw (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/ocn_sw.h"

// Stencil tile of one 256-thread workgroup (sw_kernels.hip k_range): OCN_TW columns (a
// multiple of 64) x OCN_ROWS rows; OCN_XCD_REMAP = XCD-banded tile order.
#ifndef OCN_TW
#define OCN_TW 64
#endif
#ifndef OCN_ROWS
#define OCN_ROWS 8
#endif
#ifndef OCN_XCD_REMAP
#define OCN_XCD_REMAP 1
#endif
#define OCN_WY (256 / OCN_TW)
static_assert(OCN_TW % 64 == 0 && 256 % OCN_TW == 0, "OCN_TW must be 64, 128 or 256");

#ifndef OCN_FIELD_SKEW
#define OCN_FIELD_SKEW 0
#endif
static_assert(OCN_FIELD_SKEW % 256 == 0, "OCN_FIELD_SKEW must keep fields 256-B aligned");

// Minimum waves per SIMD requested from the register allocator for the stencil kernels.
#ifndef OCN_LB_WAVES
#define OCN_LB_WAVES 1
#endif

// shared/constants.f90:23  FreeFallAcc = 9.8 (real(4))
#define OCN_FREE_FALL_ACC 9.8f

namespace ocn {

int set_error(int code, const std::string &msg);

inline bool is_r8(int id) { return id >= OCN_SSH && id < OCN_FIELD_END; }   // SW fields (tracers: ctx_has_field)
inline bool is_r4(int id) { return id >= 0 && id < OCN_NUM_R4; }
inline int field_slot(int id) { return is_r4(id) ? id : OCN_NUM_R4 + (id - OCN_SSH); }
constexpr int kNumSlots = OCN_NUM_R4 + OCN_NUM_R8;   // without tracer fields
constexpr int kMaxTracers = 64;

#ifndef OCN_RANGE_DEFINED   // also in sw_stencils.h
#define OCN_RANGE_DEFINED
struct Range { int m0, m1, n0, n1; };   // [m0, m1] x [n0, n1], 1-based global indices
#endif

// A block's compact static fields (sw_stencils.h): mask bytes (pitch x rows) and metric rows;
// march: run the stencil launches that have one as register marches (sw_kernels.hip k_march).
struct Compact {
    const uint8_t *bits;
    const float *rows;
    bool march;
};

// Fused step groups (sw_kernels.hip); `ptr` = the block's field table indexed by field_slot(),
// `cp` = its compact tables or nullptr for the 2-D real(4) arrays, `part` = which part of the
// launch range (sw_stencils.h frame_rects: the halo-overlap split).
enum { OCN_PART_ALL = 0, OCN_PART_FRAME = 1, OCN_PART_INNER = 2 };
int launch_fused_a(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int part,
                   const ocn_sw_params &sw, double tau, bool reuse, hipStream_t s);
// flip: the role-flip form (sw_kernels.hip MarchFusedB<true>: + a8's filters and check_ssh_err
// into flip_nbad on the interior; needs cp->march); rc: hhq / hhu_p / hhv_p recomputed from
// h_r, ssh, sshp (after a MarchCA<false>, which does not store them)
// up_out / vp_out / inner (one-pass calls with halo exchanges): the role-flip B on the interior
// outside *inner, a8's filtered sshp / ubrtrp / vbrtrp into sshp_out / up_out / vp_out
int launch_fused_b(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int part,
                   const ocn_sw_params &sw, double tau, bool full, bool reuse, hipStream_t s,
                   int32_t *flip_nbad = nullptr, bool flip = false, bool rc = false, double *sshp_out = nullptr,
                   double *up_out = nullptr, double *vp_out = nullptr, const Range *inner = nullptr);
// sshp_in: a8 reads sshp there and writes the table's sshp (recompute steps), nullptr = in place
int launch_fused_c1(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int part,
                    const ocn_sw_params &sw, int32_t *nbad, hipStream_t s, const double *sshp_in = nullptr,
                    const double *up_in = nullptr, const double *vp_in = nullptr);
// keep_n (march path, full): hqn / hun / hvn / hhn already hold hh_init's n level (from h_r) and
// are not stored again.  copy (march path, whole bnd range): also dst[k] := src[k] (the call tail's
// a8 copies sshn := ssh, ubrtrn := ubrtr, vbrtrn := vbrtr; src[0] the ssh hh_init reads)
struct TailCopy { const double *src[3]; double *dst[3]; };
int launch_fused_c2(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int part,
                    const ocn_sw_params &sw, bool full, hipStream_t s, bool keep_n = false,
                    const TailCopy *copy = nullptr);
// Role-flip calls: step k's hh_init (non-final) and step k+1's fused A in one launch
// (sw_kernels.hip MarchCA); next_reuse = step k+1 is a reuse step (else A's a2 stores too);
// skip_rc = step k+1 is a recompute step (hhq on the interior, hhu_p, hhv_p not stored).
// inner: only the bnd range outside *inner (the frame of a one-pass step with halo exchanges)
int launch_fused_ca(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int part,
                    const ocn_sw_params &sw, double tau_next, bool next_reuse, bool skip_rc, hipStream_t s,
                    const Range *inner = nullptr);
// floats of a block's compact row table for nrows rows: metric rows, ratios, reciprocals
// (sw_stencils.h kRowTable, recip_offset)
size_t row_table_size(unsigned nrows);

// Initial state on the device (init_kernels.hip; ctx_setup.hip init_state).  GridInit: one block's
// real(4) static fields from the basin mask (device copy, nx x ny int32, 1-based (m, n) at
// (m-1) + (n-1) nx) and the grid's row / column factors from the host's libm.
struct GridInit {
    ocn_block g;
    const int32_t *mask;
    int nx;
    float *r4[OCN_NUM_R4];
    const float *cos_t, *cos_v;                    // per row (n - bnd_y1): (float) dcosd(lat_mod(yt / yv))
    const double *sin_v, *cosy_v, *cos_xu;         // dsind(yv), dcosd(yv) per row; dcosd(xu) per column
    double cos_rot, sin_rot, sin_extr;             // dcosd / dsind(rotation_on_lat), dsind(lat_extr)
    float sx, sy, cor, sqrt2;                      // base steps (m), 2 * EarthAngVel, sqrt(2.0)
    int curve;
    // rows outside the metric range: their factors and where their metric values go (kExtRows x
    // (OCN_NUM_R4 - OCN_DX) floats: OCN_DX .. OCN_R_DISS of each; nullptr: not formed) -- rows
    // bnd_y1, bnd_y2 (the x2 steps' second ring), then bnd_y1 - 1, bnd_y1 - 2, bnd_y2 + 1, bnd_y2 + 2
    // (the x4 pairs' third and fourth rings, outside the reference's arrays)
    static constexpr int kExt = 6;
    float ext_ct[kExt], ext_cv[kExt];
    double ext_sin_v[kExt], ext_cosy_v[kExt];
    float *ext;
};
constexpr int kExtRows = GridInit::kExt;
constexpr int kExtRowFloats = kExtRows * (OCN_NUM_R4 - OCN_DX);
// Extra halo rings of every real(8) field and of the x4 mask bytes beyond the reference's 2
// (bnd_x1 - kXRing .. bnd_x2 + kXRing, bnd_y1 - kXRing .. bnd_y2 + kXRing addressable): the pair
// launches with halo exchanges read the state 4 points out (ocn_ctx.hip one_step_x4)
constexpr int kXRing = 2;
int launch_init_grid(const GridInit &q, hipStream_t s);
// gaussian_elimination_kernel (vel_ssh.f90:15-38) into p (zero outside the sea interior)
int launch_gaussian(const ocn_block &g, double *p, const float *lu, int nx0, int ny0, double sigma, hipStream_t s);
// v at every point of the block array (not the row padding)
int launch_fill_field(const ocn_block &g, double *p, double v, hipStream_t s);
// One-pass role-flip step (sw_kernels.hip MarchStep): a1 + fused B + a8's filters + check_ssh_err
// with hh_init's depths, vort and the stresses formed in registers from the state; single block,
// no a8 / a9 work on the halo ring; a8's filtered sshp / ubrtrp / vbrtrp go to the given buffers.
// range: the points it computes (default: the interior) -- with halo exchanges, the part of the
// interior whose stencils stay off the halos the exchanges fill.
// kc: which variant -- OCN_KC_GENERAL reads h_r, mu, the forcing and D's fallback values;
// OCN_KC_KNOWN takes them as +0.0 / the uniform values kc[0], kc[1] (device memory, written by
// launch_fallback_check); OCN_KC_KNOWN_HR the same but reads h_r (a non-uniform rest depth:
// topography); OCN_KC_DEVICE launches all three, each running only if the device verdict *flag
// (launch_fallback_check's: bit 0 h_r varies, bit 1 anything else) is its own -- no host wait.  The
// word after it, flag[1]: nonzero if mu's one value is not +0.0 (read by the host only).
// nv (OCN_KC_KNOWN / OCN_KC_KNOWN_HR chosen on the host): mu is +0.0 and every r_diss row +0.0f -- the
// two-step launches run their inviscid bodies (MarchStep NV: no viscous or friction terms formed)
#ifndef OCN_KC_DEFINED   // also in ocn_step_plan.h
#define OCN_KC_DEFINED
enum { OCN_KC_GENERAL = 0, OCN_KC_KNOWN = 1, OCN_KC_DEVICE = 2, OCN_KC_KNOWN_HR = 3 };
#endif
struct OnepassKC { int mode; const int32_t *flag; const double *kc; bool nv = false; };
// own (sw_stencils.h own_class bits, not with last): the halo points neighbour blocks own hold the
// neighbours' state two points deep -- D there is formed as on their interior (MarchStep X2).
// frame_of: only the part of the range outside *frame_of, as up to 4 bands in one launch
int launch_onepass(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, const ocn_sw_params &sw,
                   double tau, int32_t *nbad, double *sshp_out, double *up_out, double *vp_out, hipStream_t s,
                   const Range *range, bool last, const OnepassKC &kc, unsigned own = 0,
                   const Range *frame_of = nullptr);
// the two-step launches' fixed tile height in force (ocn_set_pair_rows / OCN_PAIR_ROWS; 0: automatic)
int pair_rows_fixed();
// Two one-pass steps in one launch (sw_kernels.hip MarchStep PAIR): single block, no exchange,
// a variant chosen on the host (kc.mode OCN_KC_KNOWN / OCN_KC_KNOWN_HR / OCN_KC_GENERAL); reads the state where a single step reads it and writes the second step's new state where
// a single step writes (one role flip); nbad1 / nbad2: the steps' check_ssh_err counts (null: none)
// last: the second step is the call's last step (MarchStep LAST: the consumers also store vort, the
// stresses and the RHS terms the reference's last step leaves)
// the pair launches' shader-clock counters (sw_kernels.hip g_clk: ticks, 100 MHz ticks, launches)
int clock_read(bool reset, unsigned long long out[3]);
int launch_onepass_pair(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, const ocn_sw_params &sw,
                        double tau, int32_t *nbad1, int32_t *nbad2, double *sshp_out, double *up_out, double *vp_out,
                        hipStream_t s, const OnepassKC &kc, bool last = false);
// Two one-pass steps per launch with halo exchanges (sw_kernels.hip MarchStep PAIR + X2; ocn_ctx.hip
// one_step_x4): bx = the block widened by kXRing rings, ptr / cp over that geometry (launch_x4_tables),
// the state exchanged 4 deep; the known-constant variant (kc.mode OCN_KC_KNOWN); own: the halo points
// neighbour blocks own; range: the consumers' points (nullptr: the interior), frame_of: only the bands
// of it outside *frame_of (one launch of up to 4 rects); nblk: blocks of this size batched into the
// launch (the tile height's cost model); trs (tracer runs): four arrays (based like the fields) that get the
// first step's new ssh, sshp, ubrtr, vbrtr on the producers' points -- the second tracer step's state
int launch_onepass_pair_x4(const ocn_block *bx, void *const *ptr, int nptr, const Compact *cp, const ocn_sw_params &sw,
                           double tau, int32_t *nbad1, int32_t *nbad2, double *sshp_out, double *up_out, double *vp_out,
                           hipStream_t s, const OnepassKC &kc, unsigned own, const Range *range = nullptr,
                           int nblk = 1, const Range *frame_of = nullptr, double *const *trs = nullptr);
// one_step_x4's tables of block g: mask bytes over g widened by kXRing (bits4, its base at
// A(bnd_x1 - kXRing, bnd_y1 - kXRing), pitch g->pitch) and the row table of those rows (rows4,
// row_table_size(rows + 2 kXRing)) from the block's own tables, its ext rows and the basin mask
// (device, nx x ny); ORs OCN_COMPACT_DIVISOR_RANGE into *flags
int launch_x4_tables(const ocn_block *g, const uint8_t *bits, const float *rows, const float *ext, uint8_t *bits4,
                     float *rows4, const int32_t *mask, int nx, int ny, unsigned own, int32_t *flags, hipStream_t s);
// nsteps one-pass steps in one launch (sw_kernels.hip k_march_multi): single small block, no
// exchange, a variant chosen on the host; step 1 reads the table's buffers, each step the buffers
// the previous one wrote (the role pairs and sshp / ubrtrp / vbrtrp against *_alt, alternating);
// ctr: kMultiBarBytes of device words for the grid barrier, at the start of their own allocation
// (zeroed on the stream first); err: ORed 1 if a barrier timed out.  onepass_multi_fits: the block's
// grid is small enough for one resident launch on the current device (its tile count against every
// variant's occupancy x the device's CUs, queried once per device).  spin: the barrier's bound on
// polls before it gives up (kMultiSpin; tests force it low to exercise the timeout path).
constexpr size_t kMultiBarBytes = 17 * 128;   // the top counter, 8 group counters, 8 group generations
constexpr int kMultiSpin = 1 << 20;           // ~0.5 s of s_sleep(1) polls
int onepass_multi_fits(const ocn_block *b);
int launch_onepass_multi(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, const ocn_sw_params &sw,
                         double tau, int nsteps, int32_t *nbad, double *sshp_alt, double *up_alt, double *vp_alt,
                         unsigned *ctr, int32_t *err, hipStream_t s, const OnepassKC &kc, int spin = kMultiSpin);
// The multi-step launch for several members of an ensemble at once (sw_kernels.hip k_march_multi_b):
// n members of one block geometry and one variant (onepass_multi_variant: the known-constant, h_r-read
// or general body, tau a power of two or not, with or without the per-step check; -1 where the host has
// not chosen one), `rows` rows per wave tile, each member's tiles one after the other in the grid.  A
// member brings its field table, compact tables, blow-up counter, second buffers, its own
// kMultiBarBytes of barrier words (zeroed on the stream first), its own timeout flag and spin bound.
// d_tab / h_tab: device and pinned host memory for the members' table (tab_bytes each, at least
// n x onepass_multi_b_entry_bytes()); the host copy is read when the stream reaches the copy.
// capacity: workgroups that may be resident (at most onepass_multi_b_capacity(), the occupancy of
// every variant of both multi-step kernels x the device's CUs): n x tiles above it is an error.
// launch_onepass_multi_ens is that launch; with `rec` the recorder is in it, with `frc` the forcing, with `peak`
// the peak update (below; `peak` with `frc` is one kernel, `rec` with either or both of the others is
// k_march_multi_all).
struct EnsMember {
    const ocn_block *b;
    void *const *ptr;
    int nptr;
    const Compact *cp;
    int32_t *nbad;
    double *alt[3];
    unsigned *ctr;
    int32_t *err;
    const double *kc;
    int spin;
    // the forcing launch alone: the member's index in the ensemble (its entry of the forcing table) and,
    // for a forced member, its second RHSx / RHSy buffers (the odd steps' table names them)
    int index = 0;
    double *frc2[2] = {nullptr, nullptr};
};
int onepass_multi_variant(int kc_mode, double tau, bool check);
size_t onepass_multi_b_entry_bytes();
long onepass_multi_b_capacity();
struct EnsLaunch {
    const EnsMember *m;
    int n, variant, rows;
    const ocn_sw_params &sw;
    double tau;
    int nsteps;
    void *d_tab, *h_tab;
    size_t tab_bytes;
    long capacity;
};
struct EnsRecLaunch;
struct EnsFrcLaunch;
struct EnsPeakLaunch;
int launch_onepass_multi_ens(const EnsLaunch &L, const EnsRecLaunch *rec, const EnsFrcLaunch *frc, hipStream_t s,
                             const EnsPeakLaunch *peak = nullptr);
// The ensemble launch with a station recorder in it (sw_kernels.hip k_march_multi_rec; ocn_sw.h
// ocn_ens_step_record): after each due step but the call's last, every member with a column >= 0 stores
// H_j of its state into slot[j * n + col], j < nobs.  The operator is one table for all the members of the
// launch (one block, one geometry): start as EnsObsOp's, term[t].slot the index of the term's field in
// `field` (nfields of the six prognostic fields), term[t].off its element.  due0: the call's first due step
// (1-based; beyond nsteps: none), then every `every` steps; slot0: the first due record's slot, the next
// nobs * n doubles on.  h_mem / d_mem: pinned host and device memory for n EnsRecMember (the host copy is
// read when the stream reaches the copy).  capacity: at most onepass_multi_rec_capacity().
struct EnsObsTerm;
struct EnsRecMember { const double *f[2][OCN_ENS_OBS_MAX_FIELDS]; int col, pad; };   // [parity of the steps done][field]
struct EnsRecArgs {
    const EnsRecMember *mem; const int *start; const EnsObsTerm *term;
    double *slot0; int due0, every, nobs, n;
};
struct EnsRecLaunch {
    const int *col; const int32_t *field; int nfields;
    const int *d_start; const EnsObsTerm *d_term;
    double *slot0; int due0, every, nobs, n;
    EnsRecMember *h_mem, *d_mem;
};
long onepass_multi_rec_capacity();
// Statistics over the members of an ensemble (ens_stats.hip; ocn_sw.h ocn_ens_stats): of the n arrays
// src[0 .. n) (one field of one block geometry in member order, all with the lane of A(bnd_x1, :) in its
// 256-B line that src[0] has) into out[0 .. 5) = mean, variance, spread, minimum, maximum (based like the
// sources; nullptr: not stored), every point of A(bnd_x1:bnd_x2, bnd_y1:bnd_y2), ONE launch.  need_var:
// the variance is formed (for out[1] or out[2]; n >= 2).  Up to kEnsStatsReg members the values stay in
// registers between the two passes.
constexpr int kEnsStatsReg = 32;
int launch_ens_stats(const ocn_block *b, const double *const *src, int n, bool need_var, double *const out[5],
                     hipStream_t s);
// Per-member extrema (ocn_ens_extrema): EnsPartial is ocn_ens_extrema_t's layout.  d_blk[k]: block k's
// interior (w x h points from element `off` of its arrays) and its first tile of the grid's x dimension
// (ens_extrema_tiles(w, h) tiles each, tiles_x of them per tile row); d_tab[member * nblk + k]: that
// member's field and lu of block k; d_part: members x ntiles partials; d_out: members results.  Two
// launches: a wave per tile and member, then a wave per member.
struct EnsPartial { double min, max; long long nonfinite, count; };
struct EnsExtBlock { long off, pitch; int w, h, first_tile, tiles_x; };
struct EnsExtSrc { const double *src; const float *lu; };
int ens_extrema_tiles(int w, int h, int *tiles_x);
int launch_ens_extrema(const EnsExtBlock *d_blk, int nblk, const EnsExtSrc *d_tab, int members, int ntiles,
                       EnsPartial *d_part, EnsPartial *d_out, hipStream_t s);
// Recombination of the members (ens_transform.hip; ocn_sw.h ocn_ens_transform): the n arrays mem[0 .. n)
// (one field of one block geometry, the members in use in member order) become their linear combinations
// by the n x n weights, at every point of A(bnd_x1:bnd_x2, bnd_y1:bnd_y2).  d_wt: the weights on the
// device, ens_wt_stride(n) x ens_wt_cols(n) doubles, the weight of old member a in new member b at
// ens_wt_index(n, a, b) and +0.0 everywhere else -- up to kEnsStatsReg members transposed (a column's
// weights side by side, kEnsStatsReg apart); beyond, per pass of 8 columns one input's 8 weights side by
// side.  Up to kEnsStatsReg members ONE launch, in place; beyond, into the staging arrays
// stage + b * stage_stride (elements; based like mem[0]) and a second launch that copies them back.
inline int ens_wt_stride(int n) { return n <= kEnsStatsReg ? kEnsStatsReg : n; }
inline int ens_wt_cols(int n) { return n <= kEnsStatsReg ? n : (n + 7) / 8 * 8; }
inline size_t ens_wt_index(int n, int a, int b)
{
    return n <= kEnsStatsReg ? (size_t)b * kEnsStatsReg + a : (size_t)(b / 8) * 8 * n + (size_t)a * 8 + b % 8;
}
int launch_ens_transform(const ocn_block *b, double *const *mem, int n, const double *d_wt, double *stage,
                         long stage_stride, hipStream_t s);
// out[p * n + m] = member m's value at point p (ocn_ens_sample): element d_off[p] of mem[m], or with
// d_tab (several blocks) of d_tab[d_blk[p] * n + m].  ONE launch.
int launch_ens_sample(const double *const *mem, const double *const *d_tab, int n, const long *d_off,
                      const int *d_blk, int npts, double *d_out, hipStream_t s);
// The localized serial observation update (ens_local.hip; ocn_sw.h ocn_ens_local_update) of the n arrays
// mem[0 .. n) (one field of one block geometry, the members in use in member order), in place, at the
// points of A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) the block's observations reach.  d_list: ngroups x kLuGroup
// entries, the block's observations in the caller's order (io, jo global; k the row of d_y and d_z), the
// last group filled up with ens_lu_filler(); d_y, d_z: the rows, ens_lu_row(n) doubles apart; d_taper:
// ntaper doubles; reach: the largest r with r * r < ntaper.  ONE launch; beyond kEnsStatsReg members the
// values live in n x 512 B of dynamic LDS.
constexpr int kLuGroup = 4;   // list entries a wave reads and tests at a time
constexpr int kLuRow = 8;     // the y and z rows are padded to a multiple of this many doubles
struct EnsLuObs { int32_t io, jo, k, pad; };
constexpr EnsLuObs ens_lu_filler() { return EnsLuObs{-(1 << 30), -(1 << 30), 0, 0}; }   // (its box meets no wave; host and device)
inline size_t ens_lu_row(int n) { return (size_t)(n + kLuRow - 1) / kLuRow * kLuRow; }
int launch_ens_local(const ocn_block *b, double *const *mem, int n, const EnsLuObs *d_list, int ngroups, const double *d_y,
                     const double *d_z, const double *d_taper, int ntaper, int reach, hipStream_t s);
// The observation-space loop of the serial filter (ens_assim.hip; ocn_sw.h ocn_ens_assimilate), every
// pointer on the device.  tab[b * n + m]: member u_m's array of the observed field on block b; observation j
// is element off[j] of block blk[j]'s arrays, at the global indices (io[j], jo[j]).  hx, y, z: nobs rows,
// row = ens_lu_row(n) doubles apart (hx: gathered, then followed through the loop; y, z: formed; their
// padding written +0.0); innovation, prior, posterior: nobs doubles; nonfinite: one count.  ONE launch of
// ONE workgroup of kAsThreads threads, whatever n and nobs.
constexpr int kAsThreads = 256;
struct EnsAsArgs {
    const double *const *tab; const long *off; const int *blk, *io, *jo;
    const double *value, *variance, *taper;
    double *hx, *y, *z, *innovation, *prior, *posterior; long *nonfinite;
    long row; int n, nobs, ntaper, reach;
};
int launch_ens_obs_space(const EnsAsArgs &a, hipStream_t s);
// A sparse linear observation operator on the device (ens_assim.hip; ocn_sw.h ocn_ens_sample_h,
// ocn_ens_assimilate_h): observation j owns the terms start[j] .. start[j+1]-1 (1 .. OCN_ENS_OBS_MAX_TERMS of
// them); term t is element off of tab[slot + m] for member u_m -- slot = (field slot * blocks + block) * n, tab
// the members' arrays field by field, block by block -- times w.  The host has validated every offset.
struct EnsObsTerm { long slot, off; double w; };
struct EnsObsOp { const double *const *tab; const int *start; const EnsObsTerm *term; };
// out[j * n + m] = H_j(member u_m), j < nobs.  ONE launch.
int launch_ens_sample_h(const EnsObsOp &h, int n, int nobs, double *d_out, hipStream_t s);
// launch_ens_obs_space with the prologue hx[j][m] = H_j(member u_m): a.tab, a.off and a.blk are not read.  ONE
// launch of ONE workgroup of kAsThreads threads.
int launch_ens_obs_space_h(const EnsAsArgs &a, const EnsObsOp &h, hipStream_t s);
// The station recorder's series as the source of hx (ens_assim.hip; ocn_sw.h ocn_ens_record_sample,
// ocn_ens_assimilate_rec): observation j reads the series at the elements obs[j].off + col[m] and, with
// obs[j].wt != 0.0, `next` further on (the same row and column of the next record) -- off = (rec * nobs_r + row) *
// n_r, next = nobs_r * n_r, col[m] the recorder's column of the m-th member in use -- and interpolates between
// them with the weight wt.  The host has validated every offset.
struct EnsRecObs { long off; double wt; };
struct EnsRecSrc { const double *series; const EnsRecObs *obs; const int *col; long next; };
// out[j * n + m] = the rule's hx[j][m], j < nobs.  ONE launch.
int launch_ens_record_sample(const EnsRecSrc &r, int n, int nobs, double *d_out, hipStream_t s);
// launch_ens_obs_space with the prologue hx[j][m] = the rule's: a.tab, a.off and a.blk are not read.  ONE launch
// of ONE workgroup of kAsThreads threads.
int launch_ens_obs_space_r(const EnsAsArgs &a, const EnsRecSrc &r, hipStream_t s);
// The gate (ocn_sw.h ocn_ens_set_gate) of the three stages above, as an argument of its own behind theirs:
// EnsAsArgs keeps its layout, so k_ens_obs_space_h's and _r's second argument stays where it is and the ungated
// kernels keep their bytes.  gate2 > 0 (+inf allowed); accept: nobs doubles, written 1.0 or 0.0; list: the
// nlist entries of all blocks' lists, the contiguous region ens_lu_put_lists uploads -- the stage's epilogue
// overwrites each entry of a rejected observation with ens_lu_filler(), and the update's launches, behind it on
// the same stream, read the rewritten lists (k_ens_local itself is unchanged).
struct EnsAsGate { double gate2; double *accept; EnsLuObs *list; int nlist; };
// launch_ens_obs_space, _h and _r with the gate in the loop: their checks, plus gate2, accept and list.  ONE
// launch of ONE workgroup of kAsThreads threads each.
int launch_ens_obs_space_g(const EnsAsArgs &a, const EnsAsGate &g, hipStream_t s);
int launch_ens_obs_space_hg(const EnsAsArgs &a, const EnsObsOp &h, const EnsAsGate &g, hipStream_t s);
int launch_ens_obs_space_rg(const EnsAsArgs &a, const EnsRecSrc &r, const EnsAsGate &g, hipStream_t s);
// Covariance inflation (ens_inflate.hip; ocn_sw.h ocn_ens_inflate) of the n arrays mem[0 .. n) (one field of
// one block geometry, the members in use in member order, n >= 2), in place, at every point of
// A(bnd_x1:bnd_x2, bnd_y1:bnd_y2).  mode: OCN_ENS_INFLATE_*; d_spread: the saved spread (RTPS; else unused);
// d_factor: the factor applied, or 1.0, at every point; both based like the members' arrays.  ONE launch;
// beyond kEnsStatsReg members the members are read once per pass.
int launch_ens_inflate(const ocn_block *b, double *const *mem, int n, int mode, double alpha, const double *d_spread,
                       double *d_factor, hipStream_t s);
// Correlated perturbations (ens_perturb.hip; ocn_sw.h ocn_ens_perturb).  launch_ens_noise: Z of one draw id
// over A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) of one block for the n members in use (members[a]: the a-th one's index
// in the ensemble) into d_z, member a's array at d_z + a * zstride, based like the members' arrays (lead: the
// lane of A(bnd_x1, :) within its 256-B line).  launch_ens_perturb_apply: the n arrays mem[0 .. n) (one field,
// member order) take c * D from that scratch, in place, where d_mask (real(4), the block's pitch; nullptr:
// everywhere) is > 0.5f.  ONE launch each.
int launch_ens_noise(const ocn_block *b, const uint8_t *members, int n, uint64_t seed, uint32_t draw, int reach, int passes,
                     long long *d_z, long zstride, int lead, hipStream_t s);
int launch_ens_perturb_apply(const ocn_block *b, double *const *mem, int n, const long long *d_z, long zstride, bool centre,
                             double c, const float *d_mask, hipStream_t s);
// The moving-storm forcing (ens_forcing.hip; ocn_sw.h ocn_ens_forcing_apply): OCN_RHSX / OCN_RHSY of every forced
// member of one block geometry for time t, at the block's interior points.  d_tab: `members` entries on the
// device, one per member of the ensemble -- its storm, its arrays of this block (the real(4) masks and metrics,
// h_r, the two outputs) and whether it is forced (others are left alone).  lead: the lane of A(bnd_x1, :) within
// its 256-B line.  ONE launch.  rx2, ry2: the member's second buffers (the forcing launch's; else null).
struct EnsFrcMember {
    ocn_ens_storm s;
    const float *lcu, *lcv, *dx, *dy, *dxt, *dyt, *dxh, *dyh;
    const double *hr;
    double *rx, *ry, *rx2, *ry2;
    int forced, pad;
};
int launch_ens_forcing(const ocn_block *b, const EnsFrcMember *d_tab, int members, const ocn_ens_forcing_model &model,
                       double t, int lead, hipStream_t s);
// The ensemble launch with the forcing formed in it (sw_kernels.hip k_march_multi_frc; ocn_sw.h
// ocn_ens_step_forced), for the general variants only: step s (0-based) of a forced member reads RHSx / RHSy from
// buffer s & 1 -- 0 the fields' own arrays, 1 the member's second pair (EnsMember::frc2) -- and between its march
// of step s and the barrier behind it every workgroup writes its share of the forcing of t0 + (double)(s + 1) tau
// into buffer (s + 1) & 1.  The caller has written the forcing of t0 into the fields' own arrays ahead of the
// launch.  d_tab: the forcing table of the block (launch_ens_forcing's), indexed by EnsMember::index; a member that
// is not forced there marches as in the plain launch.  capacity: at most onepass_multi_frc_capacity().
struct EnsFrcLaunch { const EnsFrcMember *d_tab; ocn_ens_forcing_model model; double t0; };
long onepass_multi_frc_capacity();
// The peak map (ens_peak.hip; ocn_sw.h ocn_ens_peak_*): per point the highest and / or lowest value one of the six
// prognostic fields has had after a step, and that step's number, by ens_peak_point.h.  One EnsPeakMember per
// member of a table in device memory, written by a copy ordered before the launch and never by a kernel (scalar
// loads through the constant address space): src[0] the field's array as the member's field table names it (the
// state after an even number of the launch's steps), src[1] the odd steps' table's (the marching launch alone);
// pmax / smax and pmin / smin the peaks and their steps (null: that extreme is not followed), P based like the
// field, S int32 with the same element index; tracked 0: the member is left alone.  The interior and the step
// count ride in the entry too (k0: the steps counted before the launch), so that the marching launch's hook costs
// one kernel argument.
struct EnsPeakMember {
    const double *src[2];
    double *pmax; int32_t *smax;
    double *pmin; int32_t *smin;
    long off, pitch;    // the interior's first element, the array's pitch
    int w, npts;        // the interior's width and its number of points
    int k0, tracked;
};
// launch_ens_peak: every tracked member of one block geometry, one point per lane, grid.z = member; d_tab:
// `members` entries.  k = 0: init -- P = the field, S = 0 at the interior's points; k >= 1: the rule with step k
// (the entries' k0 is not read).  lead: the lane of A(bnd_x1, :) within its 256-B line.  ONE launch.
int launch_ens_peak(const ocn_block *b, const EnsPeakMember *d_tab, int members, int k, int lead, hipStream_t s);
// out[j * w + i] = (double)c / (double)n over the block's whole array (w x h, dense), c the number of the n arrays
// pmax[0 .. n) (member order) with a value > threshold at the point (a NaN is not counted).  ONE launch.
int launch_ens_exceed(const ocn_block *b, const double *const *pmax, int n, double threshold, double *d_out, hipStream_t s);
// The ensemble launch with the peak update in it (sw_kernels.hip k_march_multi_pk): behind the barrier of every
// step but the launch's last, the workgroups of a tracked member share the interior's points and apply the rule
// with step k0 + (steps done) to the state in the table of that parity.  h_mem / d_mem: pinned host and device
// memory for the launch's n entries, in the launch's member order, the caller's part (the peaks, the interior, k0,
// tracked) filled in; the launch adds src[0] / src[1] of `field` (one of the six prognostic fields).  With `frc`
// as well the forcing is formed in the same launch (the general bodies).  capacity: at most
// onepass_multi_pk_capacity().
struct EnsPeakLaunch { int32_t field; EnsPeakMember *h_mem, *d_mem; };
long onepass_multi_pk_capacity();
// The ensemble launch with everything in it (sw_kernels.hip k_march_multi_all; ocn_sw.h ocn_ens_run): `rec` together
// with `frc` and / or `peak` -- the forcing fill ahead of each barrier, the peak update and the due records behind
// it, each as in its own launch above.  The recorder's and the peak's tables are in the launch's member order, the
// forcing's is indexed by EnsMember::index.  capacity: at most the least of the capacities of what the launch
// carries and onepass_multi_all_capacity().
long onepass_multi_all_capacity();
// the known-constant precondition of launch_onepass over r (sw_kernels.hip FallbackCheck: the
// fallback points and the forcing hold +0.0, h_r and mu are uniform): ORs 1 into *flag where it
// does not hold; writes h_r and mu at (r.m0, r.n0) to kc[0], kc[1]
int launch_fallback_check(const ocn_block *b, void *const *ptr, const uint8_t *bits, const Range &r, int32_t *flag,
                          double *kc, hipStream_t s, unsigned own = 0);
// Builds the compact tables of a block from its real(4) arrays; ORs OCN_COMPACT_* reasons
// they cannot be used into *flags (device int); own: the halo points neighbour blocks own
// (sw_stencils.h own_class bits; OCN_COMPACT_EDGE_RING_SEA tests the others)
int launch_prepare(const ocn_block *b, void *const *ptr, uint8_t *bits, float *rows, int32_t *flags, hipStream_t s,
                   unsigned own = 0);
// rows_x = the row table `rows` with rows 0 and nrows - 1 formed from ext (init_kernels.hip k_ext_rows:
// the metric values of rows bnd_y1 / bnd_y2 as the neighbours form them); ORs
// OCN_COMPACT_DIVISOR_RANGE into *flags if a divisor there is out of udiv's range
int launch_rows_ext(const ocn_block *b, const float *rows, float *rows_x, const float *ext, int32_t *flags,
                    hipStream_t s);
constexpr int kCompactEdgeRingSea = 16;   // sw_stencils.h OCN_COMPACT_EDGE_RING_SEA
// Tracer stage `stage` (OCN_TSTAGE_*) of tracer k (1-based) on one block.
// one reference stage (OCN_STAGE_*) over the compact tables: the ocn_<stage> entry's write set
// and results (sw_kernels.hip KStage; hh_init as the register march with cp->march)
int launch_stage(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int stage, const ocn_sw_params &sw,
                 double tau, int32_t *nbad, hipStream_t s);
int launch_tracer(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int stage, int k, double tau,
                  double ts, hipStream_t s);
// the three tracer stages of tracer k as one launch in a one-pass sequence (sw_stencils.h TracerStep:
// hh_init's hhu / hhv / hhq_p formed from the state): ffn into ffn_out, the filtered ffp into ffp_out;
// own: the halo points neighbour blocks own (their fluxes formed here, as the exchange delivers them);
// ext: also the first halo ring's points neighbours own, updated as those neighbours update them (x4
// pairs with tracers: the state 4 and the tracers 2 points deep exchanged)
int launch_tracer_step(const ocn_block *b, void *const *ptr, int nptr, const Compact *cp, int k, double tau,
                       double ts, double *ffn_out, double *ffp_out, unsigned own, hipStream_t s, bool ext = false);
// ORs 1 into *flags (device int) if a buffer pair of the role-flip step differs outside the
// pair's write set (sw_stencils.h Coherence).
int launch_coherence(const ocn_block *b, void *const *ptr, const uint8_t *bits, int32_t *flags, hipStream_t s);
// the same for tracer k's ff1 / ff1n (the tracer steps' role pair) outside the ring range's lu points
int launch_tracer_coherence(const ocn_block *b, void *const *ptr, const uint8_t *bits, int k, int32_t *flags,
                            hipStream_t s);
// Prepare's flag bit reporting mask bits on the halo ring (sw_stencils.h OCN_COMPACT_RING_SEA)
constexpr int kCompactRingSea = 4;
constexpr int kCompactDivisorRange = 8;   // sw_stencils.h OCN_COMPACT_DIVISOR_RANGE
constexpr int kCompactViscousRow = 32;    // sw_stencils.h OCN_COMPACT_VISCOUS_ROW

// Block batching (sw_kernels.hip): while a Batcher is active on this thread, the launches of the
// march / range / frame kernels are collected per kernel type instead of issued, and batch_end
// issues each kind for all the blocks that added one together (their tiles in one grid, up to
// kPack launch bodies by value in the kernel arguments).  A block loop of a stage launches one
// kernel per block: with several small blocks per device those launches are latency-bound.
//   batch_begin(bt, s); for each block { batch_next(bt); launches on s } batch_end(bt);
// Each block's launches keep their order (a block that adds a kind out of the batch's kind order,
// or one kind twice, flushes the batch first); launches of different blocks may be reordered, so
// a batched loop must not let one block's launch read what another block's writes.  Any other
// launch while a batch is open (another kernel, another stream) is an error (check_launch).
// co_launch: the caller states that no launch of the batch reads what another writes (a one-pass
// x2 step and the previous state's tracer step: both read the exchanged state, each writes its own
// buffers), so an entry may issue itself and the next one as ONE launch (co_flush: the x2 march's
// and the tracer step's workgroups in one grid) instead of two in order.
struct BatchEntry {
    virtual ~BatchEntry() {}
    virtual int flush(hipStream_t s) = 0;
    // issue this entry and `next` as one launch; false: not possible (each flushes on its own)
    virtual bool co_flush(BatchEntry *next, hipStream_t s, int &rc) { (void)next; (void)s; (void)rc; return false; }
    const void *kind = nullptr;   // the kernel type (its host stub's address)
};
struct Batcher {
    bool active = false;
    bool co_launch = false;              // see BatchEntry::co_flush (cleared by batch_begin)
    int co_launched = 0;                 // launches that issued two entries (the last flush)
    hipStream_t s = nullptr;
    int cur = -1;                        // position of the current block's last entry
    std::vector<BatchEntry *> entries;   // in first-added order
    int flush();                         // issue and clear the collected launches
    ~Batcher();
};
extern thread_local Batcher *g_batcher;
void batch_begin(Batcher *bt, hipStream_t s);
inline void batch_next(Batcher *bt) { if (bt) bt->cur = -1; }
int batch_end(Batcher *bt);

int check_hip(hipError_t e, const char *what);
// every kernel launch of the library is followed by check_launch(): it also counts them
// (ocn_launch_count, for the launches-per-step figure of bench.py)
void count_launch();
int batch_violation();
inline int check_launch()
{
    count_launch();
    if (g_batcher && g_batcher->active) return batch_violation();
    return check_hip(hipGetLastError(), "kernel launch");
}

}  // namespace ocn
