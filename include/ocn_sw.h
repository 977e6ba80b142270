/*
 * ocn_sw.h -- C ABI of the MI355X-native shallow-water barotropic step.
 *
 * Drop-in boundary for the reference's kernel and PSy layers
 * (Andrcraft9/ocean_model_arch; citations are path:line in that tree):
 *
 *  - Kernel layer: one entry per SW stage.  Each replaces the Fortran kernel
 *    `S(nx_start,nx_end,ny_start,ny_end,bnd_x1,bnd_x2,bnd_y1,bnd_y2,[scalars],arrays...)`
 *    (every argument by reference, explicit-shape arrays) and its CUDA-Fortran twin
 *    `S_gpu<<<grid,16x16,0,stream(k)>>>` (gpu/kernel/ *_gpu.f90).  Same argument order,
 *    same meaning, same write set, bitwise-identical results.
 *  - PSy layer: a model context that owns the per-block device storage of ocean_type /
 *    grid_type (core/ocean.f90:14-48, core/grid.f90:23-90), runs one stage plus its halo
 *    sync (envoke, core/kernel_interface.f90:48-119) or the whole step
 *    (expl_shallow_water, control/shallow_water/shallow_water.f90:22-94), and exchanges
 *    1-wide 8-direction halos (sync/hybrid_sync, shared/mpp/sync.f90:294-556) between blocks
 *    of this process and, over RCCL, with blocks of other processes (one block per GPU).
 *
 * Conventions
 *  - Indices are the reference's 1-based global Fortran indices.
 *  - Arrays are column-major A(bnd_x1:bnd_x2, bnd_y1:bnd_y2); a pointer is the DEVICE
 *    address of A(bnd_x1,bnd_y1); the leading dimension is ocn_block.pitch elements
 *    (>= bnd_x2-bnd_x1+1; r4 and r8 arrays of one block share the pitch).
 *  - `stream` is a hipStream_t passed as an opaque pointer (NULL = default stream).
 *    Entries are asynchronous on that stream; they never allocate or synchronise.
 *  - Return value: OCN_OK, or an OCN_ERR_* code (ocn_last_error() describes it).
 *    The reference kernels return nothing and ignore CUDA status; here every status is
 *    checked and reported.
 *  - No torch types; plain pointers and sizes only.
 */
#ifndef OCN_SW_H
#define OCN_SW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCN_ABI_VERSION 5

enum {
    OCN_OK = 0,
    OCN_ERR_ARG = 1,       /* bad argument (null pointer, bounds, pitch, id) */
    OCN_ERR_HIP = 2,       /* HIP runtime error */
    OCN_ERR_COMM = 3,      /* RCCL error or missing communicator */
    OCN_ERR_STATE = 4,     /* call out of order (e.g. step before init) */
    OCN_ERR_BLOWUP = 5     /* check_ssh_err: |ssh| >= 1e4 on a sea point */
};

/* Block geometry (core/decomposition.f90:40-81, block k of domain_type). */
typedef struct ocn_block {
    int32_t nx_start, nx_end, ny_start, ny_end;   /* interior (bnx_start..) */
    int32_t bnd_x1, bnd_x2, bnd_y1, bnd_y2;       /* array bounds (bbnd_x1..) */
    int64_t pitch;                                 /* leading dimension, elements */
} ocn_block;

/* ---------------------------------------------------------------- kernel layer */
/* kernel/shallow_water/vel_ssh.f90:69  sw_update_ssh_kernel */
int ocn_sw_update_ssh(const ocn_block *b, double tau,
                      const float *lu, const float *dx, const float *dy, const float *dxh, const float *dyh,
                      const double *hhu, const double *hhv, double *sshn, const double *sshp,
                      const double *ubrtr, const double *vbrtr, void *stream);

/* kernel/shallow_water/depth.f90:101  hh_update_kernel */
int ocn_hh_update(const ocn_block *b,
                  const float *lu, const float *llu, const float *llv, const float *luh,
                  const float *dx, const float *dy, const float *dxt, const float *dyt,
                  const float *dxh, const float *dyh, const float *dxb, const float *dyb,
                  double *hqn, double *hun, double *hvn, double *hhn,
                  const double *sh, const double *h_r, void *stream);

/* vel_ssh.f90:247  uv_trans_vort_kernel (nlev = 1) */
int ocn_uv_trans_vort(const ocn_block *b, const float *luu,
                      const float *dxt, const float *dyt, const float *dxb, const float *dyb,
                      const double *u, const double *v, double *vort, void *stream);

/* vel_ssh.f90:283  uv_trans_kernel (nlev = 1; hq accepted and unused, as in the reference) */
int ocn_uv_trans(const ocn_block *b, const float *lcu, const float *lcv, const float *luu,
                 const float *dxh, const float *dyh, const double *u, const double *v,
                 const double *vort, const double *hq, const double *hu, const double *hv,
                 const double *hh, double *RHSx, double *RHSy, void *stream);

/* kernel/shallow_water/mixing.f90:14  stress_components_kernel (nlev = 1) */
int ocn_stress_components(const ocn_block *b, const float *lu, const float *luu,
                          const float *dx, const float *dy, const float *dxt, const float *dyt,
                          const float *dxh, const float *dyh, const float *dxb, const float *dyb,
                          const double *u, const double *v, double *str_t, double *str_s, void *stream);

/* vel_ssh.f90:375  uv_diff2_kernel (nlev = 1; hu/hv accepted and unused, as in the reference) */
int ocn_uv_diff2(const ocn_block *b, const float *lcu, const float *lcv,
                 const float *dx, const float *dy, const float *dxt, const float *dyt,
                 const float *dxh, const float *dyh, const float *dxb, const float *dyb,
                 const double *mu, const double *str_t, const double *str_s,
                 const double *hq, const double *hu, const double *hv, const double *hh,
                 double *RHSx, double *RHSy, void *stream);

/* vel_ssh.f90:108  sw_update_uv */
int ocn_sw_update_uv(const ocn_block *b, double tau, const float *lcu, const float *lcv,
                     const float *dxt, const float *dyt, const float *dxh, const float *dyh,
                     const float *dxb, const float *dyb,
                     const double *hhu, const double *hhun, const double *hhup,
                     const double *hhv, const double *hhvn, const double *hhvp,
                     const double *hhh, const double *ssh,
                     const double *ubrtr, double *ubrtrn, const double *ubrtrp,
                     const double *vbrtr, double *vbrtrn, const double *vbrtrp,
                     const float *rdis, const float *rlh_s,
                     const double *RHSx, const double *RHSy, const double *RHSx_adv,
                     const double *RHSy_adv, const double *RHSx_dif, const double *RHSy_dif,
                     void *stream);

/* vel_ssh.f90:197  sw_next_step (writes interior + halo ring) */
int ocn_sw_next_step(const ocn_block *b, double time_smooth,
                     const float *lu, const float *lcu, const float *lcv,
                     double *ssh, double *sshn, double *sshp,
                     double *ubrtr, double *ubrtrn, double *ubrtrp,
                     double *vbrtr, double *vbrtrn, double *vbrtrp, void *stream);

/* depth.f90:164  hh_shift_kernel (time_smooth is a module variable there; an argument here) */
int ocn_hh_shift(const ocn_block *b, double time_smooth,
                 const float *lu, const float *llu, const float *llv, const float *luh,
                 double *hq, double *hqp, double *hqn, double *hu, double *hup, double *hun,
                 double *hv, double *hvp, double *hvn, double *hh, double *hhp, double *hhn,
                 void *stream);

/* depth.f90:14  hh_init_kernel (full_free_surface is a module variable there; an argument here) */
int ocn_hh_init(const ocn_block *b, int32_t full_free_surface,
                const float *lu, const float *llu, const float *llv, const float *luh,
                const float *dx, const float *dy, const float *dxt, const float *dyt,
                const float *dxh, const float *dyh, const float *dxb, const float *dyb,
                double *hq, double *hqp, double *hqn, double *hu, double *hup, double *hun,
                double *hv, double *hvp, double *hvn, double *hh, double *hhp, double *hhn,
                const double *sh, const double *shp, const double *h_r, void *stream);

/* vel_ssh.f90:40  check_ssh_err_kernel: device reduction; *nbad (device int32) += bad points */
int ocn_check_ssh_err(const ocn_block *b, const float *lu, const double *ssh, int32_t *nbad_device,
                      void *stream);

/* kernel/tracer/leapfrog_tracer.f90:13  tran_diff_fluxes_kernel (flux_x on lcu, flux_y on lcv) */
int ocn_tran_diff_fluxes(const ocn_block *b, const float *lcu, const float *lcv,
                         const float *dxt, const float *dyt, const float *dxh, const float *dyh,
                         const double *hhu, const double *hhv, const double *ff, const double *ffp,
                         const double *uu, const double *vv, const double *mu, double factor_mu,
                         double *flux_x, double *flux_y, void *stream);

/* leapfrog_tracer.f90:94  tran_diff_tracer_kernel */
int ocn_tran_diff_tracer(const ocn_block *b, const float *lu, const float *dx, const float *dy, double tau,
                         const double *hhqn, const double *hhqp, const double *flux_x, const double *flux_y,
                         const double *ffp, double *ffn, void *stream);

/* leapfrog_tracer.f90:138  tracer_next_step_kernel (writes interior + halo ring) */
int ocn_tracer_next_step(const ocn_block *b, double time_smooth, const float *lu, const double *ffn,
                         double *ffp, double *ff, void *stream);

/* ---------------------------------------------------------------- PSy layer: model context */

/* Field ids: storage of ocean_type / grid_type restricted to what the SW step touches. */
enum {
    /* real(4) */
    OCN_LU = 0, OCN_LUU, OCN_LUH, OCN_LCU, OCN_LCV, OCN_LLU, OCN_LLV,
    OCN_DX, OCN_DY, OCN_DXT, OCN_DYT, OCN_DXH, OCN_DYH, OCN_DXB, OCN_DYB, OCN_RLH_S, OCN_R_DISS,
    OCN_NUM_R4,
    /* real(8) */
    OCN_SSH = 32, OCN_SSHN, OCN_SSHP, OCN_UBRTR, OCN_UBRTRN, OCN_UBRTRP, OCN_VBRTR, OCN_VBRTRN, OCN_VBRTRP,
    OCN_HHQ, OCN_HHQ_P, OCN_HHQ_N, OCN_HHU, OCN_HHU_P, OCN_HHU_N, OCN_HHV, OCN_HHV_P, OCN_HHV_N,
    OCN_HHH, OCN_HHH_P, OCN_HHH_N, OCN_HHQ_REST, OCN_VORT, OCN_STR_T, OCN_STR_S, OCN_MU,
    OCN_RHSX, OCN_RHSY, OCN_RHSX_ADV, OCN_RHSY_ADV, OCN_RHSX_DIF, OCN_RHSY_DIF,
    OCN_FIELD_END,
    /* real(8) tracer storage (core/ocean.f90:38-41), present when ocn_sw_params.use_tracers > 0 */
    OCN_FLUX_X = OCN_FIELD_END, OCN_FLUX_Y, OCN_TRACER_BASE
};
#define OCN_NUM_R8 (OCN_FIELD_END - OCN_SSH)
/* ff1(k), ff1p(k), ff1n(k) of tracer k = 1..tracer_num */
#define OCN_FF1(k) (OCN_TRACER_BASE + 3 * ((k) - 1))
#define OCN_FF1P(k) (OCN_TRACER_BASE + 3 * ((k) - 1) + 1)
#define OCN_FF1N(k) (OCN_TRACER_BASE + 3 * ((k) - 1) + 2)

/* Stage ids, in the order of expl_shallow_water (shallow_water.f90:36-92). */
enum {
    OCN_STAGE_SW_UPDATE_SSH = 0, OCN_STAGE_HH_UPDATE, OCN_STAGE_UV_TRANS_VORT, OCN_STAGE_UV_TRANS,
    OCN_STAGE_STRESS_COMPONENTS, OCN_STAGE_UV_DIFF2, OCN_STAGE_SW_UPDATE_UV, OCN_STAGE_SW_NEXT_STEP,
    OCN_STAGE_HH_SHIFT, OCN_STAGE_HH_INIT, OCN_STAGE_CHECK_SSH_ERR, OCN_NUM_STAGES
};
/* Tracer stage ids, in the order of expl_tracer (control/tracer.f90:42-58). */
enum { OCN_TSTAGE_TRAN_DIFF_FLUXES = 0, OCN_TSTAGE_TRAN_DIFF_TRACER, OCN_TSTAGE_TRACER_NEXT_STEP, OCN_NUM_TSTAGES };

/* Basin description (configs/basinpar.f90:53-91, basin.par lines 1-18) */
typedef struct ocn_basin {
    int32_t nx, ny;
    double dxst, dyst, rlon, rlat;
    int32_t curve_grid;                 /* 0 carthesian, 1 undistorted sphere */
    double rotation_on_lon, rotation_on_lat;
} ocn_basin;

/* SW switches (configs/sw.f90:34-41, sw.par lines 1-7) */
typedef struct ocn_sw_params {
    int32_t full_free_surface, trans_terms, ksw_lat;
    double time_smooth, lvisc_2;
    int32_t use_tracers, tracer_num;
} ocn_sw_params;

/* Decomposition request (parallel.par + _DD_MANUAL_BLOCK_GRID_, decomposition.f90:856-858) */
typedef struct ocn_decomp {
    int32_t bnx, bny;        /* block grid (total, not per process) */
    int32_t nranks, rank;    /* processes; blocks are dealt by create_uniform_decomposition */
    int32_t device;          /* HIP device of this process */
} ocn_decomp;

/* Per-block information returned to hosts (block k of this process, k = 0..count-1). */
typedef struct ocn_block_info {
    ocn_block geom;
    int32_t bm, bn;                       /* block coordinates in the block grid (1-based) */
    int32_t nbr_rank[8];                  /* rank of neighbour in dirs 1..8 (kernel_macros.fi:4-12); -1 land, -2 outside */
    int32_t nbr_k[8];                     /* local index on that rank, or -1 */
} ocn_block_info;

typedef struct ocn_ctx ocn_ctx;

/* Host-only (no GPU needed): the blocks rank dec->rank owns, as ocn_ctx_create would make them.
 * Writes min(count, cap) entries; *count = number of blocks. */
int ocn_decompose(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask,
                  ocn_block_info *out, int32_t cap, int32_t *count);

/* Host-only schedule of one halo exchange of the real(8) fields `field_ids` for rank dec->rank:
 * the copies/messages ocn_ctx_sync performs (syncborder_block2D_gen_all.fi semantics).
 * LOCAL: strip src of local block k_src -> strip dst of local block k.
 * SEND : strip src of local block k_src -> message to `peer` at element `offset`.
 * RECV : message from `peer` at element `offset` -> strip dst of local block k.
 * Rects are inclusive global 1-based indices; strips are walked column-major. */
enum { OCN_HALO_LOCAL = 0, OCN_HALO_SEND = 1, OCN_HALO_RECV = 2 };
typedef struct ocn_halo_msg {
    int32_t kind, peer, k, k_src, field;
    int32_t dst_x0, dst_x1, dst_y0, dst_y1;
    int32_t src_x0, src_x1, src_y0, src_y1;
    int32_t count;
    int64_t offset;
} ocn_halo_msg;
int ocn_halo_schedule(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask,
                      const int32_t *field_ids, int32_t nfields, ocn_halo_msg *out, int32_t cap,
                      int32_t *count);
/* The same for the exchanges of the x2 steps (depth 2) and the x4 pairs (depth 4), as the device path
 * plans them: every side strip `depth` columns / rows deep, layer by layer, and depth x depth corner
 * patches as rows; tracer fields (ids from OCN_TRACER_BASE) go 1 deep, 2 deep in a 4-deep exchange.
 * depth 1 is ocn_halo_schedule; any other depth than 1, 2 or 4 is OCN_ERR_ARG.  The strips of a
 * neighbour narrower than the depth reach into that neighbour's own halo (the step machine runs such
 * exchanges only for h_r's copy). */
int ocn_halo_schedule_deep(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask,
                           const int32_t *field_ids, int32_t nfields, int32_t depth, ocn_halo_msg *out,
                           int32_t cap, int32_t *count);

/* Create a context: decomposes the basin (mask = int32 global (nx,ny) column-major, 0 = sea,
 * 1 = land, or NULL for the closed box of tools/io.f90:49-59), allocates every field of every
 * local block on `device` (zero-filled, as data_types.f90:517-533). */
int ocn_ctx_create(const ocn_basin *basin, const ocn_sw_params *sw, const ocn_decomp *dec,
                   const int32_t *mask, ocn_ctx **out);
int ocn_ctx_destroy(ocn_ctx *ctx);

int ocn_ctx_block_count(const ocn_ctx *ctx);
int ocn_ctx_block_info(const ocn_ctx *ctx, int k, ocn_block_info *out);
/* Device pointer of field `id` of local block k (element (bnd_x1,bnd_y1)); NULL on error. */
void *ocn_ctx_field(const ocn_ctx *ctx, int k, int id);
/* Compute stream of the context (hipStream_t). */
void *ocn_ctx_stream(const ocn_ctx *ctx);

/* RCCL: unique id (128 bytes) made on rank 0, broadcast by the host, then attached. */
int ocn_comm_unique_id(void *out_id, int32_t nbytes);
int ocn_ctx_attach_comm(ocn_ctx *ctx, const void *unique_id, int32_t nbytes);
/* Test transport: the n ranks of one decomposition as n contexts of ONE process on one device (n >= 1)
 * (ctxs[i] = rank i of nranks = n), each then driven by its own host thread.  Replaces only the
 * RCCL calls (the per-peer ncclRecv/ncclSend of an exchange become device copies between the
 * contexts' message buffers behind event handshakes; the role-flip vote's ncclAllReduce a device
 * max over the contexts); every other part of the multi-rank path is the production one.  Call
 * before ocn_ctx_init_state; the contexts may be destroyed in any order. */
int ocn_ctx_attach_loopback(ocn_ctx *const *ctxs, int32_t n);

/* What a multi-rank run reports about its transport (bench.py's `rccl` object): transport 0 = none,
 * 1 = RCCL (nccl_version = ncclGetVersion, comm_size / comm_rank = ncclCommCount /
 * ncclCommUserRank), 2 = loopback; exchanges = halo exchanges with remote peers enqueued so far (one
 * ncclGroupStart ... ncclGroupEnd group each), exchanges_done = the id of the last of them whose end
 * the device has reached (polled from events while a watchdog is set, else -1). */
typedef struct ocn_comm_info {
    int32_t transport, nccl_version, comm_size, comm_rank;
    int64_t exchanges, exchanges_done;
    double watchdog_s;
} ocn_comm_info;
int ocn_ctx_comm_info(ocn_ctx *ctx, ocn_comm_info *out);
/* The x2 / x4 steps' overlap with OCN_OPT_OVERLAP auto (-1) and peers on other ranks: the first step
 * of a sequence's kind (not the one that opens it) runs exchange-then-march, the next the inner part
 * beside the exchange, each timed with events; the next vote max-reduces both times over the ranks
 * and every rank keeps the faster form.  Each kind keeps its own pair of measurements (a call that
 * mixes x4 pairs with a single x2 step loses neither); the first kind every rank has measured in both
 * forms decides the level of both.  An x4 pair is measured only where every block of the grid, on any
 * rank, keeps an inner part (the same answer on every rank).  After OCN_OVERLAP_MAX_VOTES (6) votes
 * without a decision -- calls too short to hold a step that may be timed, ranks that keep disagreeing --
 * the choice gives up: level 2, the default before there was a measurement, and no further probe.
 * level = the OCN_OPT_OVERLAP level in effect; state 0 = nothing measured, 1 = the sequential step
 * measured, 2 = both (not yet voted) -- of the kind measured last --, 3 = decided, 4 = gave up
 * (level 2); 3 and 4 are final until OCN_OPT_OVERLAP is set again; kind = the form measured last or
 * decided from (2: x2 steps, 4: x4 pairs); probes = the steps run as timed probes so far (none once
 * the state is final); seq_ms / overlapped_ms = the times (after the decision: the maxima over the
 * ranks it used).  The reference's hybrid overlap mode (core/kernel_interface.f90:105-117) has no
 * such choice. */
#define OCN_OVERLAP_MAX_VOTES 6
typedef struct ocn_overlap_info {
    int32_t level, state, kind, probes;
    double seq_ms, overlapped_ms;
} ocn_overlap_info;
int ocn_ctx_overlap_info(ocn_ctx *ctx, ocn_overlap_info *out);
/* The shader clock the two-step launches (the dominant kernel: MarchStep pairs) ran at, measured in
 * the kernel: workgroup 0 of every pair launch counts the s_memtime ticks and the 100 MHz
 * s_memrealtime ticks over its tiles.  launches = pair launches sampled, clock_ghz = the ticks'
 * ratio (0 with none), sampled_ms = the real time sampled.  Device-wide (every context on the
 * context's device) since the last reset; reset != 0 zeroes the counters after reading them.
 * Synchronises the context's stream.  Telemetry only: no counterpart in the reference. */
typedef struct ocn_clock_info {
    int64_t launches;
    double clock_ghz, sampled_ms;
} ocn_clock_info;
int ocn_ctx_clock_info(ocn_ctx *ctx, int32_t reset, ocn_clock_info *out);
/* Host-side watchdog (seconds > 0; 0 = off): a thread of the context watches every call that may
 * take part in a collective (init_state, step, complete, synchronize, sync, stage, tracer_stage,
 * download, upload, output_r4).  One that has not returned after `seconds` is ended: the watchdog
 * prints "ocn watchdog: rank R of N: <call> ... last completed exchange id D of E" to stderr, aborts
 * the RCCL communicator (ncclCommAbort: RCCL's kernels waiting on a peer exit) or fails the loopback
 * group, and the call returns OCN_ERR_COMM with that message; if it still has not returned 10 s
 * later, the watchdog ends the process with exit status 3 (no exec).  The reference's analogue is
 * abort_model -> mpi_abort (shared/errors.f90:30-37), which has no timeout of its own. */
int ocn_ctx_set_watchdog(ocn_ctx *ctx, double seconds);

/* Bottom topography (basin.par line 20, control/init_data.f90:111-121): the real(4) file's values,
 * the (nx-4) x (ny-4) interior points in Fortran order (tools/io.f90:84-176 read_data2D_real4);
 * h = NULL: none (100 m everywhere).  Used by the next ocn_ctx_init_state. */
int ocn_ctx_set_topography(ocn_ctx *ctx, const float *h, int64_t count);
/* Initial state: init_grid_data + init_ocean_data (control/init_data.f90:29-125). */
int ocn_ctx_init_state(ocn_ctx *ctx);

/* sync(domain, field) for one field over all local blocks (+ remote neighbours). */
int ocn_ctx_sync(ocn_ctx *ctx, int field_id);
/* envoke(stage): the stage on every local block, then its sync list (sw_interface.f90). */
int ocn_ctx_stage(ocn_ctx *ctx, int stage_id, double tau);
/* envoke of tracer stage `stage_id` (OCN_TSTAGE_*) for tracer k (1-based, data_id), then its
 * sync list (interface/tracer/tracer_interface.f90). */
int ocn_ctx_tracer_stage(ocn_ctx *ctx, int stage_id, int tracer, double tau);
/* nsteps model steps (model.f90:146-160): expl_shallow_water(tau), then expl_tracer(tau) when
 * use_tracers > 0.  check_every: run check_ssh_err every N steps (0 = never). */
int ocn_ctx_step(ocn_ctx *ctx, double tau, int32_t nsteps, int32_t check_every);
/* Wait for the context's stream; returns OCN_ERR_BLOWUP if a check found |ssh| >= 1e4, and
 * OCN_ERR_HIP if a multi-step launch's grid barrier timed out since the last synchronize (the
 * results are invalid; ocn_ctx_init_state starts over).  With a communicator attached (RCCL or
 * loopback) this is a COLLECTIVE: the blow-up counts are max-reduced over the ranks
 * (check_ssh_err_kernel -> abort_model stops every rank, shared/errors.f90:30-37), so every rank
 * must call it, in the same order relative to its steps; a rank that skips it leaves the others
 * waiting in the reduction. */
int ocn_ctx_synchronize(ocn_ctx *ctx);
/* Form a pending call tail now (OCN_OPT_LAZY_TAIL): afterwards every array holds what the
 * reference leaves after the last step run.  Every entry that reads or writes fields, hands out a
 * pointer, runs a stage or a sync, or sets an option does this first; a host that reads device
 * memory by other means calls it itself.  Asynchronous on the context stream. */
int ocn_ctx_complete(ocn_ctx *ctx);

/* Host <-> device copies of a whole field of local block k (host array: Fortran order,
 * leading dim bnd_x2-bnd_x1+1, 4 or 8 bytes per element by field kind). Synchronous. */
int ocn_ctx_download(ocn_ctx *ctx, int k, int field_id, void *host);
int ocn_ctx_upload(ocn_ctx *ctx, int k, int field_id, const void *host);
/* Output record of one field of local block k (control/output.f90:32-174 bufwp4%copy_from_real8
 * + tools/io.f90:276-386 write_data2D_real4): the interior nx_start..nx_end x ny_start..ny_end,
 * Fortran order, as real(4) (round to nearest from real(8)), with `undef` where |lu| < 0.5.
 * Converted on the device; host receives (nx_end-nx_start+1)*(ny_end-ny_start+1) floats. Synchronous. */
int ocn_ctx_output_r4(ocn_ctx *ctx, int k, int field_id, float undef, float *host);

/* Execution options.
 *  OCN_OPT_GRAPH: replay each step as one hipGraph (single-process runs).
 *  OCN_OPT_OVERLAP (default -1 = auto): with halo exchanges, run each exchange on a second stream
 *  beside the launches' inner parts (points that neither read halos nor feed the exchange): 1 = in
 *  the standard steps and in the one-pass steps (there the frame launches and both exchanges as one
 *  chain on the second stream beside the whole inner march), 2 = in the role-flip steps too,
 *  0 = never (same results bit for bit); auto
 *  is 2 when the context exchanges with other ranks (RCCL or loopback attached, nranks > 1), else
 *  1.  ocn_ctx_get_option returns the level in effect.
 *  OCN_OPT_STAGE_TIMING: bracket every launch group with HIP events on the context stream.
 *  OCN_OPT_FUSED (default 1): ocn_ctx_step runs the step as 4 fused launch groups and 3 halo
 *  syncs (same results and final state bit for bit); 0 = the 11 envoke stages of the reference.
 *  OCN_OPT_COMPACT (default 1): the fused step -- and the reference stages run by ocn_ctx_step
 *  with OCN_OPT_FUSED 0 or by ocn_ctx_stage -- read the real(4) masks as one bit-packed byte
 *  per point and the grid metrics as one value per row, when that is exact for the current
 *  real(4) fields (checked when they were last set; same results bit for bit).  Handing out a
 *  real(4) pointer with ocn_ctx_field disables this until it is set to 1 again, which also
 *  rebuilds the tables from the fields at the next ocn_ctx_step.
 *  OCN_OPT_MARCH (default 1): with the compact tables, the stencil launches that have a
 *  register-march form (fused A, fused B, hh_init) run as one (same results bit for bit);
 *  0 = one thread per point.
 *  OCN_OPT_FLIP (default 1): with compact tables and march, no tracers: every step of an
 *  ocn_ctx_step call but the last replaces sw_next_step's copies (ssh := sshn, ubrtr := ubrtrn,
 *  vbrtr := vbrtrn) by swapping the two buffers of each pair inside the library, and runs its
 *  time filters inside fused B (same results bit for bit; the pointers of ocn_ctx_field are the
 *  same after the call).  Needs the pairs to agree outside their write sets and, with halo
 *  exchanges, the halo ring of ssh, ubrtr, vbrtr, hhu, hhv, hhq_rest to hold the neighbours'
 *  values; both hold from ocn_ctx_init_state on and are checked on the device whenever fields
 *  were uploaded or handed out (with an RCCL communicator: at every call, all ranks deciding
 *  together); otherwise the standard step runs.
 *  OCN_OPT_RECOMPUTE (default 1): in such calls (full_free_surface = 1, no a8 / a9 work on the
 *  halo ring, so one block without halo exchanges), steps 2..K-1 form hhq, hhu_p, hhv_p inside
 *  fused B instead of storing and re-reading them (same results bit for bit).
 *  OCN_OPT_ONEPASS (default 1): in such calls with trans_terms and ksw_lat on and no tracers,
 *  steps 2..K-1 run as one launch each: the state is read once and the next state written once,
 *  hh_init's depths, vort and the stresses formed in registers (same results bit for bit; takes
 *  precedence over OCN_OPT_RECOMPUTE).  Step 1 too when nothing changed the state since the
 *  last hh_init; on one block without halo exchanges and a8 / a9 work on the halo ring, the last
 *  step as well; with halo exchanges, the bands along the exchanged sides run the role-flip path.
 *  OCN_OPT_KNOWN_CONSTANTS (default 1): the one-pass steps take the forcing and D's fallback
 *  values as zero and h_r, mu as uniform constants when a check of the arrays (at the first
 *  one-pass call, and after any field is handed in) finds them so; 0: always the general variant.
 *  OCN_OPT_ONEPASS_LAST (default 1): with halo exchanges or a8 / a9 work on the halo ring, the
 *  call's last step as a one-pass step too (the inner march storing what the reference's last
 *  step leaves, then a8's copies and hh_init with every level); 0: a standard last step there.
 *  OCN_OPT_LAZY_TAIL (default 1): in one process (one block without halo exchanges, or the blocks of
 *  OCN_OPT_X2 steps), no tracers and no raw real(8) pointer handed out, a call whose steps are one-pass steps leaves its tail (what
 *  the reference's last step stores beyond the next state: vort, the stresses, the RHS terms,
 *  sw_next_step's copies, hh_init with every level) pending: the next ocn_ctx_step continues with
 *  one-pass steps -- so 1-step calls (the reference's own cadence, model.f90:146) run as fast as
 *  long ones -- and ocn_ctx_complete, or any entry that looks at the fields, forms it first (the
 *  last step run again from the previous state, which is still in the library's second buffers:
 *  the same results bit for bit).  ocn_ctx_get_option returns 2 while a tail is pending.
 *  OCN_OPT_X2 (default 1): with halo exchanges (several blocks or ranks), the one-pass steps
 *  exchange the state (ssh, sshp, ubrtr, ubrtrp, vbrtr, vbrtrp) two points deep, once per step, and
 *  form the depths, vort and stresses on the halo themselves, so the march covers the whole
 *  interior (one exchange per step instead of two, no frame launches); needs the real(4) fields
 *  from ocn_ctx_init_state, blocks of at least 2 x 2 points, no a8 / a9 work on a halo ring no
 *  neighbour fills, and OCN_OPT_ONEPASS_LAST; the second halo ring, which the reference never
 *  writes, is restored before the call's last step (same results bit for bit).  ocn_ctx_get_option:
 *  whether the last ocn_ctx_step used such steps.  Lazy call tails (OCN_OPT_LAZY_TAIL) apply to them
 *  too when the context exchanges only with blocks of its own process.
 *  OCN_OPT_BATCH (default 1): with several blocks on the device, each launch group of a step is
 *  issued once for all of them (the blocks' tiles in one grid) instead of once per block.
 *  OCN_OPT_PAIR (default 1): two one-pass steps in one launch where both are plain one-pass steps
 *  of a single-block context without exchanges, the one-pass variant is chosen on the host (a
 *  known-constant verdict the host read, or the general variant), and the second is not the call's
 *  last step run -- the first step's new state stays on chip (98 B per cell for two steps in the
 *  known-constant variant); 1: the known-constant variants on blocks of at least 512 x 512 interior
 *  points, 2: any variant on any block, 0: never.  Same results bit for bit.  ocn_ctx_get_option: 2 if the last
 *  ocn_ctx_step ran such launches, else whether the option is on.
 *  OCN_OPT_MULTI (default 1): in an open sequence (OCN_OPT_LAZY_TAIL) without pairs, all steps of a
 *  call in ONE launch with a grid-wide barrier between the steps, where the block is small
 *  enough for its whole grid to be resident (the launch-latency-bound case: the Black Sea basin as one
 *  block), single block without exchanges, the variant chosen on the host, check_every 0 or 1, no
 *  graph replay.  Same results bit for bit.  ocn_ctx_get_option: 2 if the last ocn_ctx_step ran one.
 *  OCN_OPT_TRACER_STEP (default 1): tracer runs (use_tracers) with one-pass steps -- each step's
 *  expl_tracer as one launch per tracer that forms hh_init's depths it reads from the state, run with
 *  the next step (after its exchange, which carries the tracers one point deep); the call's last step
 *  runs the standard tracer stages.  Needs the call's first step to be a one-pass step, and with
 *  exchanges the x2 steps; no graph replay.  Same results bit for bit.  ocn_ctx_get_option: 2 if the
 *  last ocn_ctx_step used them.
 *  OCN_OPT_X4 (default 1): with halo exchanges, x2 steps run two per launch with ONE exchange of the
 *  state four points deep per two steps (the launch's first step also updates the two halo rings
 *  neighbour blocks own, as they do) -- the pair launch of single blocks (OCN_OPT_PAIR) for blocks with
 *  neighbours; the known-constant variant, every block at least 4 x 4; two more halo rings outside the
 *  reference's arrays hold the exchanged state.  Tracer runs (tracer steps): the tracers exchanged two
 *  deep, two tracer steps per exchange -- with 1 only where exchanges go to other ranks, with 3 always.
 *  0 = off.  Same results bit for bit.  ocn_ctx_get_option: 2 if the last ocn_ctx_step used such
 *  launches, else the value set (0, 1 or 3).
 *  OCN_OPT_CO_LAUNCH (default 1): tracer runs with x2 steps (one tracer, block batching on): each
 *  step's march -- with OCN_OPT_OVERLAP 2 the part after the exchange -- and the previous state's
 *  tracer step go as ONE launch (their workgroups in one grid) instead of two.  Same results bit for
 *  bit.  ocn_ctx_get_option: 2 if the last ocn_ctx_step co-launched.
 *  OCN_OPT_INVISCID (default 1): the two-step launches (OCN_OPT_PAIR, OCN_OPT_X4) of the known-constant
 *  variants form none of the viscous (a5 stresses, a6 uv_diff2) and bottom-friction terms where the
 *  checks find the viscosity mu +0.0 everywhere and r_diss +0.0f in every row, as ocn_ctx_init_state
 *  leaves them: every such term is then +-0 and the momentum sums are the same bit for bit; rows whose
 *  state is not finite and below 2^300 are computed in full.  Dropped, like the known-constant variant,
 *  whenever a field is handed in or a raw real(8) pointer handed out, until the next check.  Same
 *  results bit for bit.  ocn_ctx_get_option: 2 if the last ocn_ctx_step ran such launches.
 *  OCN_OPT_MULTI_SPIN (diagnostics; default 1 << 20, about 0.5 s): the multi-step launch's grid
 *  barrier gives up after this many polls -- the launch's workgroups end and ocn_ctx_synchronize
 *  returns OCN_ERR_HIP instead of the device hanging if the grid was not co-resident.  Tests set it
 *  to 1 to exercise that path.
 *  OCN_OPT_XCHG_DELAY (tests; default 0): microseconds the device waits before each exchange with
 *  remote peers (a slow link, for the measured overlap choice: ocn_ctx_overlap_info).
 * ocn_ctx_get_option: current value; for OCN_OPT_COMPACT whether the last ocn_ctx_step used
 * the compact tables, for OCN_OPT_FLIP whether it used role-flip steps, for OCN_OPT_RECOMPUTE
 * whether it used recompute steps, for OCN_OPT_ONEPASS whether it used one-pass steps (2: with
 * the forcing and fallback values known to be zero and h_r, mu known to be uniform, taken as
 * kernel constants instead of being read; 3: the same with h_r read -- a non-uniform rest depth,
 * e.g. a topography file). */
int ocn_ctx_set_option(ocn_ctx *ctx, int32_t key, int64_t value);
int ocn_ctx_get_option(const ocn_ctx *ctx, int32_t key, int64_t *value);
enum { OCN_OPT_GRAPH = 1, OCN_OPT_OVERLAP = 2, OCN_OPT_STAGE_TIMING = 3, OCN_OPT_FUSED = 4, OCN_OPT_COMPACT = 5,
       OCN_OPT_MARCH = 6, OCN_OPT_FLIP = 7, OCN_OPT_RECOMPUTE = 8, OCN_OPT_ONEPASS = 9,
       OCN_OPT_KNOWN_CONSTANTS = 10, OCN_OPT_ONEPASS_LAST = 11, OCN_OPT_LAZY_TAIL = 12, OCN_OPT_X2 = 13,
       OCN_OPT_BATCH = 14, OCN_OPT_PAIR = 15, OCN_OPT_MULTI = 16, OCN_OPT_TRACER_STEP = 17,
       OCN_OPT_MULTI_SPIN = 18, OCN_OPT_X4 = 19, OCN_OPT_CO_LAUNCH = 20, OCN_OPT_XCHG_DELAY = 21,
       OCN_OPT_INVISCID = 22 };

/* Timer slots: the stage ids, then the fused groups (fused C2 is OCN_STAGE_HH_INIT), then the
 * three tracer stages (summed over tracers), then the role-flip steps' fused hh_init + next A,
 * then the one-pass steps: one step, two steps per launch, two steps the second of which is the
 * call's last (the tail of an open sequence, ocn_ctx_complete), several steps in one launch
 * (OCN_OPT_MULTI), the tracer step of one-pass sequences (OCN_OPT_TRACER_STEP), then the halo
 * exchanges with remote peers and the exposed part of the overlapped ones (ocn_ctx_stage_stats). */
enum { OCN_TIMER_FUSED_A = OCN_NUM_STAGES, OCN_TIMER_FUSED_B, OCN_TIMER_FUSED_C1, OCN_TIMER_TRACER,
       OCN_TIMER_FUSED_CA = OCN_TIMER_TRACER + OCN_NUM_TSTAGES, OCN_TIMER_ONEPASS, OCN_TIMER_ONEPASS2,
       OCN_TIMER_ONEPASS2_LAST, OCN_TIMER_ONEPASS_MULTI, OCN_TIMER_TRACER_STEP, OCN_TIMER_EXCHANGE,
       OCN_TIMER_EXPOSED, OCN_NUM_TIMERS };

/* Per-timer device time (ms, summed) and launch counts since the last call, from the HIP
 * events of OCN_OPT_STAGE_TIMING; arrays of OCN_NUM_TIMERS entries.  Synchronises. */
int ocn_ctx_stage_times(ocn_ctx *ctx, double *ms, int64_t *counts);
/* The same, plus the longest single record per timer (ms_max; may be NULL).  OCN_TIMER_EXCHANGE:
 * one halo exchange with remote peers (pack, the RCCL group / loopback copies, unpack) on the
 * stream that runs it; OCN_TIMER_EXPOSED: per overlapped step, how long the comm stream's chain
 * (exchange + frame march) outlasted the compute stream's inner march -- the part of the exchange
 * not hidden (0 when hidden). */
int ocn_ctx_stage_stats(ocn_ctx *ctx, double *ms, int64_t *counts, double *ms_max);

/* ---------------------------------------------------------------- ensembles
 * Members of one small basin stepped together: N contexts of the same basin, mask and decomposition on
 * one device, whose multi-step launches (OCN_OPT_MULTI) go as ONE launch per group of members, each
 * member with a grid barrier of its own inside it -- a basin of the Black Sea's size fills a tenth of
 * the device, and its step is bound by the barrier, which the members of a launch pay side by side.
 * No counterpart in the reference (one process runs one model).
 *
 * ocn_ens_plan (pure, no device; the policy ocn_ens_step uses): how `members` members of block `geom`
 * go into launches of at most `capacity` workgroups.  variant[i] >= 0 names member i's kernel variant
 * (members of one launch share it); variant[i] < 0: not eligible, in no group.  A member at `rows`
 * rows per wave tile has ceil(W / 60) * ceil(H / (4 rows)) tiles (W x H the block's interior).  Per
 * variant, in ascending order of the id: the smallest rows in 1..16 at which all its members fit the
 * capacity together, as one group; if none does, rows = 16 and groups of floor(capacity / tiles)
 * members in member order.  A block with more tiles than the capacity at 16 rows is in no group.
 * *count = the groups (all of them, also beyond cap); out[0 .. min(cap, *count)) is written.  A
 * group's members are member[0 .. members), ascending; member j's first workgroup in the grid is
 * first_tile[j] = j * tiles.  members is at most OCN_ENS_MAX_MEMBERS (OCN_ERR_ARG beyond). */
#define OCN_ENS_MAX_MEMBERS 256
typedef struct ocn_ens_group {
    int32_t variant, rows, tiles, members;
    int32_t member[OCN_ENS_MAX_MEMBERS];
    int32_t first_tile[OCN_ENS_MAX_MEMBERS];
} ocn_ens_group;
int ocn_ens_plan(const ocn_block *geom, const int32_t *variant, int32_t members, int64_t capacity, ocn_ens_group *out,
                 int32_t cap, int32_t *count);

/* `members` (1..OCN_ENS_MAX_MEMBERS) contexts of the same basin, parameters, mask and decomposition on dec->device,
 * sharing one compute stream.  dec->nranks must be 1 (OCN_ERR_ARG otherwise); any block grid and
 * tracer count is accepted (such members are stepped one by one).  Each member owns its fields and
 * its static tables (nothing is shared: a member costs what a context costs). */
typedef struct ocn_ens ocn_ens;
int ocn_ens_create(const ocn_basin *basin, const ocn_sw_params *sw, const ocn_decomp *dec, const int32_t *mask,
                   int32_t members, ocn_ens **out);
/* Destroys the members too: their borrowed handles are invalid afterwards. */
int ocn_ens_destroy(ocn_ens *ens);
/* Number of members (-1: null). */
int ocn_ens_size(const ocn_ens *ens);
/* Member i as a BORROWED context: every ocn_ctx_* entry works on it (upload, download, field, options,
 * topography, output_r4, init_state, ocn_ctx_step for that member alone, ...) except
 * ocn_ctx_destroy, ocn_ctx_attach_comm and ocn_ctx_attach_loopback, which return OCN_ERR_ARG: the
 * ensemble owns it.  ocn_ctx_stream returns the shared stream.  OCN_ERR_ARG on a bad index. */
int ocn_ens_member(ocn_ens *ens, int32_t i, ocn_ctx **out);
/* ocn_ctx_init_state on every member. */
int ocn_ens_init_state(ocn_ens *ens);
/* ocn_ctx_step(member, tau, nsteps, check_every) for every member, with exactly its results.  The
 * members that would run their own multi-step launch in this call (an open sequence, OCN_OPT_MULTI's
 * conditions, nsteps >= 2, a variant chosen on the host) are grouped by ocn_ens_plan over the
 * capacity (below) and issued as one launch per group; every other member -- the first call after
 * an init or upload, 1-step calls, blocks too large, block grids, tracers, OCN_OPT_MULTI off, a raw
 * pointer handed out -- gets ocn_ctx_step.  Residency: every workgroup of a launch must be on the
 * device at once, so a group has at most capacity / tiles members; the capacity is the occupancy of
 * the multi-step kernels x the device's CUs, lowered by OCN_ENS_OPT_CAPACITY.  Asynchronous.  Returns
 * the first error of any member. */
int ocn_ens_step(ocn_ens *ens, double tau, int32_t nsteps, int32_t check_every);
/* ocn_ctx_complete on every member. */
int ocn_ens_complete(ocn_ens *ens);
/* Waits for the shared stream once; status[i] (may be NULL) = what ocn_ctx_synchronize returns for
 * member i: OCN_OK, OCN_ERR_BLOWUP (its check found |ssh| >= 1e4), OCN_ERR_HIP (its barrier timed
 * out: its results are invalid).  A member's blow-up or timeout neither stops nor disturbs the
 * others.  Returns the first status that is not OCN_OK. */
int ocn_ens_synchronize(ocn_ens *ens, int32_t *status);
/* The last ocn_ens_step: groups = batched launches issued, batched = members in them, rows / tiles =
 * rows per wave tile and tiles per member of the largest group (most members; 0 with none),
 * max_group = its members, capacity = the capacity in effect (workgroups). */
typedef struct ocn_ens_info_t {
    int32_t members, groups, batched, rows, tiles, max_group;
    int64_t capacity;
} ocn_ens_info_t;
int ocn_ens_info(ocn_ens *ens, ocn_ens_info_t *out);
/* OCN_ENS_OPT_CAPACITY: a cap on the workgroups of one ensemble launch (value >= 1; 0 = none).  It
 * only ever lowers the device's capacity: for a host that shares the device, and for tests, which
 * reach taller tiles and several groups on tiny blocks with it.
 * OCN_ENS_OPT_MAX_GROUP (measurements; 0 = none): at most this many of the members planned in a call go
 * to ocn_ens_plan together (in member order), so that several shorter launches can be timed against
 * one taller one (scripts/ens_bench.py). */
enum { OCN_ENS_OPT_CAPACITY = 1, OCN_ENS_OPT_MAX_GROUP = 2, OCN_ENS_OPT_ASSIM_TIMING = 3,
       OCN_ENS_OPT_RECORD_IN_LAUNCH = 4 /* ocn_ens_step_record below: 1 (default) or 0 */,
       OCN_ENS_OPT_FORCING_IN_LAUNCH = 5 /* ocn_ens_step_forced below: 1 (default) or 0 */ };
int ocn_ens_set_option(ocn_ens *ens, int32_t key, int64_t value);

/* Statistics over the members, formed on the device (the members' fields lie side by side in device
 * memory with one geometry and one pitch: N reads and one write per point instead of N downloads).
 * No counterpart in the reference.
 *
 * ocn_ens_stats: the per-point statistics `what` (OCN_ENS_STAT_* bits) of real(8) field `field_id` of
 * local block k over the members in use (use[i] != 0, i < ocn_ens_size; NULL = all), at every point of
 * A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) -- interior and halo, land and sea, whatever they hold -- all from ONE
 * launch.  With the members in use in member order u0 < u1 < ... < u(n-1) and x_i member u_i's value:
 *   MEAN    s = x0; s = s + x_i for i = 1 .. n-1 in that order; mean = s / (double)n
 *   VAR     d_i = x_i - mean; q = d0 d0; q = q + d_i d_i for i = 1 .. n-1 (the product rounded, then the
 *           sum); var = q / (double)(n-1)
 *   SPREAD  sqrt(var) (formed from the variance whether or not VAR is asked for)
 *   MIN     c = x0; for i = 1 .. n-1: if (x_i < c || c != c) c = x_i        MAX: the same with >
 *           (a tie, +-0 included, keeps the earlier member's bits; a NaN is dropped as soon as a later
 *           member has a number; all NaN gives NaN)
 * in IEEE double arithmetic without contraction: bitwise reproducible.  It first forms the pending call
 * tail of every member in use (as every entry that looks at fields does; a member not in use is not
 * touched), then launches on the ensemble's stream into buffers the ensemble owns (one per statistic and
 * block, in the members' layout, allocated at first use, freed by ocn_ens_destroy).  Each member's array
 * is the one its field table names at the time of the call.  No pointer is handed out: the members'
 * options, known-constant verdicts and raw-pointer state stay as they were, and the next ocn_ens_step
 * opens its sequences again as after ocn_ens_complete.  Asynchronous.  OCN_ERR_ARG -- nothing launched,
 * earlier results kept -- for a null ensemble, a bad k, a real(4) field or one the members do not have,
 * `what` 0 or with unknown bits, no member in use, VAR / SPREAD with fewer than two members in use.
 *
 * ocn_ens_stats_download: the whole array of one statistic (one OCN_ENS_STAT_* bit) of block k, in
 * ocn_ctx_download's layout.  ocn_ens_stats_output_r4: its packed interior as real(4) with `undef` where
 * member 0's lu says land, in ocn_ctx_output_r4's layout.  Both synchronous; OCN_ERR_STATE for a
 * statistic the last ocn_ens_stats on that block did not form.
 *
 * ocn_ens_extrema: per member (out: ocn_ens_size entries), over the interior sea points
 * (nx_start..nx_end x ny_start..ny_end with |lu| >= 0.5, the member's own lu) of real(8) field `field_id`
 * on all local blocks: min / max over the finite values (+Inf / -Inf with none; the sign of a zero is
 * unspecified), nonfinite = the NaN and +-Inf among them, count = the sea points.  Completes every
 * member; two launches for the whole ensemble; synchronous. */
enum { OCN_ENS_STAT_MEAN = 1, OCN_ENS_STAT_VAR = 2, OCN_ENS_STAT_SPREAD = 4, OCN_ENS_STAT_MIN = 8, OCN_ENS_STAT_MAX = 16 };
int ocn_ens_stats(ocn_ens *ens, int32_t k, int32_t field_id, const uint8_t *use, int32_t what);
int ocn_ens_stats_download(ocn_ens *ens, int32_t k, int32_t stat, double *host);
int ocn_ens_stats_output_r4(ocn_ens *ens, int32_t k, int32_t stat, float undef, float *host);
typedef struct ocn_ens_extrema_t { double min, max; int64_t nonfinite, count; } ocn_ens_extrema_t;
int ocn_ens_extrema(ocn_ens *ens, int32_t field_id, ocn_ens_extrema_t *out);

/* Sampling and recombining the members on the device: what a host needs to inflate, recentre, resample or
 * filter an ensemble between calls (each new member a linear combination of the old ones; the N x N
 * algebra that finds the weights stays with the host).  No counterpart in the reference.  In both entries
 * the members in use are u0 < u1 < ... < u(n-1), in member order (use[i] != 0, i < ocn_ens_size; NULL =
 * all), as in ocn_ens_stats.
 *
 * ocn_ens_sample (the observation operator): host[p * n + m] = member u_m's value of real(8) field
 * `field_id` at point p -- local block k[p], the library's 1-based global indices (i[p], j[p]), anywhere
 * within A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) of that block (halo and land included), for p < npts.  It first
 * forms the pending call tail of every member in use (a member not in use is not touched), takes each
 * member's array from its field table at that moment, gathers with ONE launch on the ensemble's stream
 * and brings the npts x n doubles down through pinned memory with one wait.  Synchronous.  No pointer is
 * handed out: options, known-constant verdicts, raw-pointer state and lazy tails stay as they were, as
 * after ocn_ens_stats.  OCN_ERR_ARG -- nothing launched, nothing written to host -- for a null argument,
 * npts < 1 or > 65536, a bad k, a point outside its block's array, a real(4) field or one the members do
 * not have, no member in use.
 *
 * ocn_ens_transform (the recombination): w is an n x n row-major host array, w[a * n + b] the weight of
 * old member u_a in new member u_b.  For every field of field_ids[0 .. nfields), every local block and
 * every point of A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) (row padding and the extra rings are neither read nor
 * written), with x_a member u_a's old value -- all new values are formed from the old ones:
 *   new_b = +0.0 if column b has no weight with a nonzero bit pattern below the sign; otherwise, over a
 *   ascending, skipping every a whose w[a][b] is +0.0 or -0.0:
 *     first kept term:  s = x_a * w[a][b]
 *     later kept terms: p = x_a * w[a][b]; s = s + p     (the product rounded, then the sum)
 *   new_b = s
 * in IEEE double arithmetic without contraction: bitwise reproducible.  A skipped term is not formed, so a
 * unit column is a bit-for-bit copy (-0 included; permutations and resampling are exact), and a member
 * whose weights are all zero -- one that blew up, say -- puts no NaN into any other member.
 * Before the launches the pending call tail of every member in use is formed; a member not in use is not
 * touched.  Up to 32 members in use the transform is in place, one launch per field and block; beyond,
 * the results go through staging arrays the ensemble owns (one per member in use, in the members' layout,
 * allocated at first use, freed by ocn_ens_destroy) and are copied back on the same stream.  Afterwards
 * each transformed field of each member in use counts as UPLOADED, with exactly ocn_ctx_upload's
 * bookkeeping, and nothing else is re-formed: the depths, vort, the stresses and every other derived field
 * stay as they were, as after an upload of the same fields, and the next step is whatever the library runs
 * after uploads (a full first step that forms the depths from the new state).  A host that transforms
 * only part of the state (ssh without sshp, say) gets what uploading that part gives.  Asynchronous on the
 * ensemble's stream; the caller's w may be reused when the call returns.  OCN_ERR_ARG -- nothing launched,
 * no member's state or bookkeeping touched -- for a null ensemble, list or w, nfields < 1, an id that is
 * real(4), absent or repeated, no member in use, a weight that is not finite. */
int ocn_ens_sample(ocn_ens *ens, int32_t field_id, const uint8_t *use, int32_t npts, const int32_t *k,
                   const int32_t *i, const int32_t *j, double *host);
int ocn_ens_transform(ocn_ens *ens, const int32_t *field_ids, int32_t nfields, const uint8_t *use, const double *w);

/* The localized serial observation update: the per-point operation of a serial square-root filter (serial
 * EnSRF, EAKF) with a distance taper, on the device.  ocn_ens_transform applies ONE weight matrix to every
 * point, a global analysis; here each state point is regressed on one observation's ensemble anomalies
 * after another, scaled by a taper of its distance to the observation.  The n-sized algebra in observation
 * space (y and z below) is the caller's here; ocn_ens_assimilate (below) forms it on the device, so a whole
 * analysis may stay there.  No counterpart in the reference.
 *
 * The members in use are u0 < u1 < ... < u(n-1) in member order (use as in ocn_ens_stats), n >= 2.
 * Observation k < nobs sits at the library's 1-based global indices (io[k], jo[k]), 1 <= io <= nx and
 * 1 <= jo <= ny of the basin; it need not lie in any local block's array.  y and z are nobs x n row-major
 * host arrays of finite doubles.  taper has ntaper finite doubles, 1 <= ntaper <= 65536, and is indexed by
 * the squared index distance d2 = (i - io)^2 + (j - jo)^2: the host chooses the taper's shape, the device
 * takes no square root.  Distances are in the index space of the field's own array: the half-cell stagger
 * of u and v points against h points is ignored, and there is no wrap-around.
 *
 * For every field of field_ids[0 .. nfields), every local block and every point (i, j) -- global indices --
 * of A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) (row padding and the extra rings are neither read nor written), with
 * x_m member u_m's current value, the observations taken in ascending k:
 *   d2 = (i-io[k])^2 + (j-jo[k])^2;  if d2 >= ntaper: skip k;  rho = taper[d2];  if rho is +0.0 or -0.0: skip k
 *   s = x_0;  s = s + x_m (m = 1 .. n-1, in that order);  mean = s / (double)n
 *   a = (x_0 - mean) * y[k][0];  then for m = 1 .. n-1:  p = (x_m - mean) * y[k][m];  a = a + p
 *   g = rho * a
 *   x_m = x_m + g * z[k][m]  for every m     (the product rounded, then the sum)
 * in IEEE double arithmetic without contraction: bitwise reproducible.  A skipped observation forms
 * nothing; a point no observation reaches is not written; a reached point has all n values written.
 *   Composition: two calls with the lists L1, then L2, give the bits of one call with L1 followed by L2
 *   (so a host splits a list longer than 8192).
 *   Halo coherence: a halo point and the neighbour block's interior point with the same global indices
 *   get the same operations; if they held the same bits before, they hold the same bits after.
 *   NaN or Inf: a member that holds one at a point poisons every member at that point (through the mean).
 *   The host leaves that member out with `use`; ocn_ens_extrema tells which one it is.
 * The bookkeeping is ocn_ens_transform's: the pending call tail of every member in use is formed first, a
 * member not in use is not touched, afterwards each listed field of each member in use counts as UPLOADED
 * and nothing else is re-formed.  One launch per field and block that an observation's reach meets
 * (values in registers up to 32 members in use, in LDS beyond).  Asynchronous on the ensemble's stream;
 * the caller's arrays may be reused when the call returns.  OCN_ERR_ARG -- nothing launched, no member's
 * tail, state or bookkeeping touched -- for a null argument, nfields < 1, an id that is real(4), absent or
 * repeated, n < 2, nobs < 1 or > 8192, an observation outside the basin, ntaper < 1 or > 65536, a y, z or
 * taper value that is not finite. */
int ocn_ens_local_update(ocn_ens *ens, const int32_t *field_ids, int32_t nfields, const uint8_t *use,
                         int32_t nobs, const int32_t *io, const int32_t *jo,
                         const double *y, const double *z, const double *taper, int32_t ntaper);

/* The serial ensemble square-root filter (Whitaker & Hamill 2002) with a taper, whole, on the device: the
 * gather at the observed points, the observation-space loop that forms the rows y and z, and
 * ocn_ens_local_update's field update with them, on the ensemble's stream with no host wait in between.
 * No counterpart in the reference.
 *
 * Members, field_ids, use, io, jo, taper and ntaper are ocn_ens_local_update's, n >= 2.  Observation j < nobs
 * is `value[j]`, with error variance `variance[j]` (finite, > 0), of real(8) field `obs_field` (which need
 * not be among field_ids) at (io[j], jo[j]), read in the local block whose interior holds the point, else
 * the first whose array A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) does.
 *   Prologue: hx[j][m] = member u_m's value at observation j (what ocn_ens_sample returns for it);
 *     prior_spread[j] = SPREAD(hx[j]) by ocn_ens_stats' definitions (ordered sum, / (double)n, d = x - mean,
 *     q = d0 * d0, q = q + d * d, / (double)(n-1), sqrt).
 *   Loop, k ascending, on the CURRENT row x = hx[k]:
 *     s1 = x_0;  s1 = s1 + x_m (m = 1 .. n-1);  ybar = s1 / (double)n;  y'_m = x_m - ybar
 *     q = y'_0 * y'_0;  then p = y'_m * y'_m, q = q + p;  s = q / (double)(n-1)
 *     D = s + r_k;  d = value_k - ybar;  t = r_k / D;  alpha = 1.0 / (1.0 + sqrt(t));  c = (double)(n-1) * D
 *     Y[k][m] = y'_m;  Z[k][m] = (d - alpha * y'_m) / c;  innovation[k] = d
 *     every row j (k itself included) then takes observation k by ocn_ens_local_update's rule, as the state
 *     point (io[j], jo[j]) with rho = taper[(io[j]-io[k])^2 + (jo[j]-jo[k])^2] (skipped if out of range or
 *     +-0.0): the rows stay what the fields hold at the observed points if obs_field is among field_ids.
 *   Epilogue: posterior_spread[j] = SPREAD(final hx[j]); the fields field_ids of every block take the nobs
 *     observations with the rows Y, Z: the bits ocn_ens_local_update(..., Y, Z, ...) gives, with all of that
 *     entry's bookkeeping (tails of the members in use formed first, a member not in use untouched, each
 *     listed field UPLOADED afterwards, nothing else re-formed).
 * IEEE double arithmetic without contraction, every product rounded before the sum, IEEE division and
 * sqrt: bitwise reproducible (ens_local_rule.ensrf_obs_space_ordered restates it in numpy).  A non-finite
 * row value, D or d propagates, as in the update; `nonfinite` counts the observations whose D or d was not
 * finite, and the remedy is the update's: ocn_ens_extrema, then `use`.
 * Launches: one for the prologue, the loop and the epilogue together, whatever n and nobs, then the
 * update's one per field and block an observation's reach meets.  Asynchronous on the ensemble's stream; the
 * caller's arrays may be reused when the call returns.  OCN_ERR_ARG -- nothing launched, no member's tail,
 * state or bookkeeping touched, the earlier results kept -- for every case ocn_ens_local_update refuses
 * (its y and z apart), an obs_field that is real(4) or absent, a value that is not finite, a variance that
 * is not finite and > 0, an observation in no local block's array.
 *
 * The results stay in the ensemble's buffers until the next ocn_ens_assimilate.  ocn_ens_assimilate_info:
 * the last successful call's counts.  ocn_ens_assimilate_result: one of its arrays into `host` -- HX (the
 * final rows), Y, Z: nobs x n row-major, unpadded; INNOVATION, PRIOR_SPREAD, POSTERIOR_SPREAD: nobs.  Both
 * wait for the stream; OCN_ERR_ARG for a null argument, an unknown `what`, or no successful call yet.
 * Measurements: with OCN_ENS_OPT_ASSIM_TIMING 1 (ocn_ens_set_option; default 0) a call records events around its
 * stages, and SPANS gives host[0], host[1] = the milliseconds of the observation-space launch and of the
 * update's launches of that call (OCN_ERR_ARG if the last call was not timed). */
int ocn_ens_assimilate(ocn_ens *ens, int32_t obs_field, const int32_t *field_ids, int32_t nfields, const uint8_t *use,
                       int32_t nobs, const int32_t *io, const int32_t *jo, const double *value, const double *variance,
                       const double *taper, int32_t ntaper);
typedef struct ocn_ens_assim_info_t { int32_t nobs, n; int64_t nonfinite; } ocn_ens_assim_info_t;
int ocn_ens_assimilate_info(ocn_ens *ens, ocn_ens_assim_info_t *out);
enum { OCN_ENS_ASSIM_HX = 0, OCN_ENS_ASSIM_Y = 1, OCN_ENS_ASSIM_Z = 2, OCN_ENS_ASSIM_INNOVATION = 3,
       OCN_ENS_ASSIM_PRIOR_SPREAD = 4, OCN_ENS_ASSIM_POSTERIOR_SPREAD = 5, OCN_ENS_ASSIM_SPANS = 6,
       OCN_ENS_ASSIM_ACCEPTED = 8 /* (7 stays an unknown `what`: OCN_ERR_ARG) */ };
int ocn_ens_assimilate_result(ocn_ens *ens, int32_t what, double *host);

/* Quality control of the observations against the background, inside the loop of ocn_ens_assimilate,
 * ocn_ens_assimilate_h and ocn_ens_assimilate_rec (below): a tide gauge that spikes has an innovation of tens of
 * background standard deviations and would drag every field within reach; a member that is NaN at an observed
 * point would write NaN there.  No counterpart in the reference.
 *
 * ocn_ens_set_gate: gate2 is the squared threshold in units of the innovation variance (9.0: 3 sigma).  0.0, of
 * either sign, turns the gate off -- the default; the three entries then launch exactly what they launch without
 * this entry.  Otherwise gate2 > 0 and not NaN; +inf is allowed and rejects only on a D or d that is not finite.
 * Anything else: OCN_ERR_ARG, the setting unchanged.  The setting holds for the three entries until it is changed.
 *   The loop with the gate on: after D and d of observation k are formed (unchanged operations, on the CURRENT
 *   row), lim = gate2 * D (one rounded product) and ok = isfinite(D) && isfinite(d) && d * d <= lim.
 *     ok: everything as without a gate.
 *     not ok, the observation is REJECTED: Y[k][m] = y'_m as formed, Z[k][m] = +0.0, innovation[k] = d, `nonfinite`
 *     counts as ever; no row takes observation k and no field point takes it.  A rejected observation forms
 *     nothing: a -0.0 stays -0.0, and a point that only rejected observations reach is not stored.
 *   prior_spread and posterior_spread keep their definitions (a rejected row's posterior is still that row's final
 *   spread).  The test is against the CURRENT row -- as observations 0 .. k-1 left it -- not against the
 *   prologue's prior: like the rest of the serial loop it depends on the ORDER of the observations (an outlier
 *   ahead of a good observation at the same point is judged against the wider, earlier background).
 * Launches: those of the ungated call, the observation-space stage still ONE launch of one workgroup; the
 * update's launches go out as before -- the host does not know what was rejected; the stage rewrites the entries of
 * rejected observations in the update's lists on the device, and the update skips them.  Asynchronous as before,
 * no new wait.  The three entries refuse what they refused: a value that is not finite is still OCN_ERR_ARG on the
 * host; the gate is for outliers and for members that are not finite.
 * (ens_local_rule.ensrf_obs_space_ordered(..., gate2=) restates it in numpy.)
 *
 * ocn_ens_assimilate_result(..., OCN_ENS_ASSIM_ACCEPTED, host): nobs doubles, 1.0 (accepted) or 0.0 (rejected);
 * all 1.0 after a call made with the gate off.  ocn_ens_gate_info: the setting, and the rejected observations of
 * the last successful call of the three entries (0 with the gate off or before any call; waits for the stream). */
int ocn_ens_set_gate(ocn_ens *ens, double gate2);
typedef struct ocn_ens_gate_info_t { double gate2; int64_t rejected; } ocn_ens_gate_info_t;
int ocn_ens_gate_info(ocn_ens *ens, ocn_ens_gate_info_t *out);

/* Observations that are not one field's value at one grid point -- an altimeter track between h points, a
 * radial velocity cos(theta) u + sin(theta) v of interpolated values, a footprint average: a SPARSE LINEAR
 * observation operator H, a CSR table over nobs observations.  No counterpart in the reference.
 *   start[0 .. nobs], start[0] = 0: observation j owns the terms start[j] .. start[j+1]-1, between 1 and
 *   OCN_ENS_OBS_MAX_TERMS of them.  Term t is (tfield[t], ti[t], tj[t], tw[t]): a real(8) field id, the
 *   library's 1-based global indices, a weight that is finite and not +-0.0.  At most OCN_ENS_OBS_MAX_FIELDS
 *   distinct fields among the terms of one call.  Each term's point is read in the local block whose
 *   interior holds it, else the first whose array A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) does (halo and land
 *   included); the terms of one observation may lie in different blocks.
 *   H_j(u) = s, where  s = x_0 * w_0;  then for the later terms in the caller's order  p = x_t * w_t;  s = s + p
 *   (x_t member u's value at term t) in IEEE double arithmetic without contraction, every product rounded
 *   before the sum: bitwise reproducible (ens_obs_rule.apply restates it in numpy), and a one-term row of
 *   weight 1.0 is a bit-for-bit copy.
 *
 * ocn_ens_sample_h: host[j * n + m] = H_j(member u_m), the members in use in member order.  Everything else
 * is ocn_ens_sample's: the pending call tail of every member in use is formed first, ONE launch, the
 * nobs x n doubles come down through pinned memory with one wait, synchronous, no bookkeeping touched;
 * OCN_ERR_ARG -- nothing launched, nothing written to host -- for a null argument, nobs < 1 or > 65536, no
 * member in use and every table error listed below.
 *
 * ocn_ens_assimilate_h: ocn_ens_assimilate with the prologue hx[j][m] = H_j(member u_m) (there is no
 * obs_field).  (io[j], jo[j]) is now the observation's ANCHOR: its localization centre in index space,
 * anywhere within the basin, not tied to its terms (the nearest point of the field that matters most, say;
 * the true position is then at most 0.71 cells away).  The loop and the epilogue are ocn_ens_assimilate's:
 * row j takes observation k with rho = taper[(io[j]-io[k])^2 + (jo[j]-jo[k])^2], and the fields field_ids
 * take the nobs observations with the rows Y, Z at the anchors, with ocn_ens_local_update's bits and
 * bookkeeping.  The rows are an AUGMENTED STATE: nobs scalars carried through the loop by the update's rule
 * at their anchors.  With a taper that is 1.0 everywhere they remain H of the updated fields (to rounding:
 * the rule is linear in the state); with any other taper H of the updated fields weighs each term's point
 * by ITS distance from observation k, the row by its anchor's, and HX is NOT what ocn_ens_sample_h gives
 * afterwards.  A list of more than 8192 observations therefore does not compose bit for bit out of two
 * calls, and nobs > 8192 is refused as before.  Launches: one for the prologue, the loop and the epilogue
 * together, then the update's.  Asynchronous on the ensemble's stream; the caller's arrays may be reused when
 * the call returns.  ocn_ens_assimilate_info and ocn_ens_assimilate_result serve the last successful call of
 * either entry.  OCN_ERR_ARG -- nothing launched, no member's tail, state or bookkeeping touched, the earlier
 * results kept -- for every case ocn_ens_assimilate refuses (its obs_field apart, the anchors in the
 * observations' place) and for: start[0] != 0, an observation with 0 or more than OCN_ENS_OBS_MAX_TERMS
 * terms, a weight that is zero or not finite, a term's field that is real(4) or absent, more than
 * OCN_ENS_OBS_MAX_FIELDS distinct fields, a term in no local block's array. */
#define OCN_ENS_OBS_MAX_TERMS 16
#define OCN_ENS_OBS_MAX_FIELDS 4
int ocn_ens_sample_h(ocn_ens *ens, const uint8_t *use, int32_t nobs, const int32_t *start, const int32_t *tfield,
                     const int32_t *ti, const int32_t *tj, const double *tw, double *host);
int ocn_ens_assimilate_h(ocn_ens *ens, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t nobs,
                         const int32_t *io, const int32_t *jo, const int32_t *start, const int32_t *tfield,
                         const int32_t *ti, const int32_t *tj, const double *tw, const double *value,
                         const double *variance, const double *taper, int32_t ntaper);

/* Station time series: the members' values at tide gauges or buoys as a function of time, and the model's
 * equivalents of observations taken during the forecast window, recorded while the members step -- INSIDE
 * the multi-step launch where there is one.  No counterpart in the reference.
 *
 * ocn_ens_record_begin starts a recorder: the operator is ocn_ens_sample_h's CSR table with the same
 * validation and the same ordered sum H_j(u), but its terms may name only the six prognostic fields (ssh,
 * sshp, ubrtr, ubrtrp, vbrtr, vbrtrp: everything else is formed by a call's tail only); the members in use
 * are u0 < u1 < ... < u(n-1) in member order (use as in ocn_ens_stats).  The series -- max_records x nobs x n
 * doubles, at most 1 GiB -- lives in a buffer the ensemble owns until ocn_ens_record_end, ocn_ens_destroy
 * or the next ocn_ens_record_begin.  Synchronous.
 *
 * ocn_ens_step_record(tau, nsteps, check_every) leaves every member exactly as ocn_ens_step with the same
 * arguments would -- the same bits, the same statuses -- and counts its steps since ocn_ens_record_begin:
 * after the counted step (r + 1) * every it writes record r,
 *   series[(r * nobs + j) * n + m] = H_j(member u_m's state after that step),
 * the state the CPU oracle holds after as many step(tau) calls, which is also what ocn_ens_sample_h returns
 * after as many ocn_ens_step(tau, 1).  Asynchronous on the ensemble's stream, no host wait.  Where every
 * member in use plans a multi-step launch for the call (an open sequence, a variant chosen on the host, one
 * small block, check_every 0 or 1, at least 2 steps: as ocn_ens_step batches them) and lands in a group
 * under the recording launches' own resident capacity, the records are written by the marching launch
 * itself, after the barrier behind each due step, and the call's last step's by ONE gather launch behind it.
 * Otherwise -- also with OCN_ENS_OPT_RECORD_IN_LAUNCH 0 (tests, measurements) -- the call is chunked: up to
 * each due step an ocn_ens_step, then one gather launch from the members' current arrays (no tail is formed:
 * the six fields are current after every call; the checks stay at the steps s of the call with
 * s % check_every == 0).  The bits of the series and of the members do not
 * depend on the route.  ocn_ens_step, ocn_ens_assimilate, ocn_ens_perturb, ocn_ens_inflate, ocn_ens_transform
 * and uploads while a recorder is active neither count nor record: a series may span analysis windows.
 * A member whose status at ocn_ens_synchronize is not OCN_OK has undefined columns from that call on; the
 * other members' columns are unaffected.  Columns are not cleared beforehand.
 *
 * ocn_ens_record_info: in_launch is the number of records written by a marching launch itself, cumulative
 * (which route ran).  ocn_ens_record_download: records first .. first + count - 1 to host, synchronous.
 * ocn_ens_record_due: the schedule alone, pure (no device, as ocn_ens_plan): the 1-based steps s of a call of
 * nsteps steps made after `counted` counted steps at which a record is due, (counted + s) % every == 0, in
 * rising order; *count their number, the first min(cap, *count) of them in steps.
 *
 * OCN_ERR_ARG -- nothing stepped, launched or written, an earlier recorder kept -- for a null argument, every
 * case ocn_ens_sample_h refuses, a term's field that is not one of the six, every < 1, max_records < 1, a
 * series above 1 GiB, an ocn_ens_step_record whose due records would pass max_records, a download range
 * outside the records taken, and for ocn_ens_record_due counted < 0, nsteps < 0, every < 1, cap < 0 or cap > 0
 * without steps.  OCN_ERR_STATE for ocn_ens_step_record, ocn_ens_record_download or ocn_ens_record_end
 * without a recorder. */
typedef struct ocn_ens_record_info_t {
    int32_t active, nobs, n, every, max_records, pad;
    int64_t steps, records, in_launch;
} ocn_ens_record_info_t;
int ocn_ens_record_begin(ocn_ens *ens, const uint8_t *use, int32_t nobs, const int32_t *start, const int32_t *tfield,
                         const int32_t *ti, const int32_t *tj, const double *tw, int32_t every, int32_t max_records);
int ocn_ens_step_record(ocn_ens *ens, double tau, int32_t nsteps, int32_t check_every);
int ocn_ens_record_info(ocn_ens *ens, ocn_ens_record_info_t *out);
int ocn_ens_record_download(ocn_ens *ens, int32_t first, int32_t count, double *host);
int ocn_ens_record_end(ocn_ens *ens);
int ocn_ens_record_due(int64_t counted, int32_t nsteps, int32_t every, int32_t *steps, int32_t cap, int32_t *count);

/* Observations at their own times: first guess at appropriate time, the asynchronous ensemble filter (Sakov
 * et al. 2010).  A tide gauge reports through the analysis window, an altimeter pass crosses the basin once
 * somewhere in it; the innovation of such an observation is value - H(state at the OBSERVATION's time), and the
 * recorder's series holds exactly those equivalents.  One gather in time, from the series on the device, in front
 * of ocn_ens_assimilate_h's loop and update, which then apply the resulting Y and Z to the state at analysis
 * time.  No counterpart in the reference.
 *
 * The rule.  An active recorder has R records taken, nobs_r rows and n_r member columns.  Observation j < nobs of
 * a call names a row row[j] of the recorder's operator (0 .. nobs_r-1), a record rec[j] (0 .. R-1) and a weight
 * wt[j], finite, 0.0 <= wt < 1.0; if wt[j] != 0.0 record rec[j] + 1 must exist as well.  With
 * a = series[rec][row][col] and b = series[rec+1][row][col]:
 *   hx[j][m] = a                                   if wt == 0.0 (a copy, bit for bit, -0.0 and NaN included; b is
 *                                                  not read)
 *            = a + q,  where p = b - a;  q = wt * p   otherwise (IEEE double, every operation rounded, no
 *                                                  contraction: ens_record_rule.interp restates it in numpy)
 * Several observations may name the same row: a gauge's readings through the window name one row at different
 * times.  The members of the call are `use`: NULL means the recorder's members, otherwise a subset of them,
 * n >= 2 either way; column m is the recorder's column of the m-th member in use, in member order.  Record r was
 * taken after the counted step (r + 1) * every: an observation at the counted step s (which may lie between
 * steps) has x = s / every - 1.0, rec = floor(x), wt = x - rec (ens_record_rule.at_steps).
 *
 * ocn_ens_record_sample: host[j * n + m] = hx[j][m].  ONE launch, the nobs x n doubles come down through pinned
 * memory with one wait; synchronous.  At most 65536 observations.  No member is read, no tail formed, no
 * bookkeeping touched: the series is already on the ensemble's stream.
 *
 * ocn_ens_assimilate_rec: ocn_ens_assimilate_h with the prologue hx[j][m] = the rule's in the place of H_j(member
 * u_m); (io[j], jo[j]) are the anchors as there.  The loop, the epilogue, the field update and all bookkeeping are
 * ocn_ens_assimilate_h's, at most 8192 observations, asynchronous on the ensemble's stream, one launch for the
 * prologue, the loop and the epilogue together and then the update's; ocn_ens_assimilate_info and
 * ocn_ens_assimilate_result serve the last successful call of the three entries.  The recorder stays active and
 * unchanged: the call neither counts nor records.
 *
 * What the caller must see to: the call uses the records AS THEY ARE.  A record taken before an earlier analysis,
 * perturbation or upload of the same window describes a trajectory the members have left: it is stale, and
 * nothing here notices.  A member whose status was not OCN_OK has undefined columns (above); the remedy is `use`.
 *
 * OCN_ERR_STATE without a recorder.  OCN_ERR_ARG -- nothing launched, no member's tail, state or bookkeeping
 * touched, the recorder and the earlier results kept, nothing written to host -- for a null argument, everything
 * ocn_ens_assimilate refuses (its obs_field apart; ocn_ens_record_sample: nobs < 1 or > 65536), no record taken
 * yet, a row or rec out of range, a wt that is not finite, < 0 or >= 1, a wt != 0 at the last record, a member in
 * `use` that the recorder does not hold, fewer than 2 members. */
int ocn_ens_record_sample(ocn_ens *ens, const uint8_t *use, int32_t nobs, const int32_t *row, const int32_t *rec,
                          const double *wt, double *host);
int ocn_ens_assimilate_rec(ocn_ens *ens, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t nobs,
                           const int32_t *io, const int32_t *jo, const int32_t *row, const int32_t *rec,
                           const double *wt, const double *value, const double *variance, const double *taper,
                           int32_t ntaper);

/* Covariance inflation on the device: what keeps a square-root filter's spread from collapsing over the
 * cycles.  ocn_ens_transform can apply ONE factor to every point (n^2 work per point, and it inflates the
 * points no observation reached as well); relaxation to prior spread (RTPS, Whitaker & Hamill 2012) needs a
 * factor per point: the analysis spread is pulled back toward the spread the ensemble had before the
 * analysis.  A cycle is ocn_ens_step, ocn_ens_spread_save, ocn_ens_assimilate, ocn_ens_inflate, ocn_ens_step:
 * asynchronous calls on the ensemble's stream with no host wait.  No counterpart in the reference.
 *
 * In both entries the members in use are u0 < u1 < ... < u(n-1) in member order (use as in ocn_ens_stats),
 * n >= 2, the fields are field_ids[0 .. nfields), real(8) only, every local block is processed at every
 * point of A(bnd_x1:bnd_x2, bnd_y1:bnd_y2) (row padding and the extra rings are neither read nor written),
 * the pending call tail of every member in use is formed first and a member not in use is not touched.
 *
 * ocn_ens_spread_save: for each listed field and block, SPREAD by ocn_ens_stats' definition, bit for bit,
 * over the members in use, into a buffer the ensemble owns (one per field and block, in the members' layout,
 * allocated at first use, freed by ocn_ens_destroy), and it remembers per field which members were in use.
 * It writes no member: nothing counts as uploaded.  One launch per field and block.  A saved spread stays
 * valid until the next save of that field.
 *
 * ocn_ens_inflate: per field, block and point, with x_m member u_m's value -- each line one IEEE double
 * operation, no contraction, products rounded before sums, IEEE division and sqrt:
 *   s = x_0;  s = s + x_m (m = 1 .. n-1);  mean = s / (double)n
 *   d_m = x_m - mean
 *   q = d_0 d_0;  p = d_m d_m, q = q + p (m = 1 .. n-1);  var = q / (double)(n-1);  sa = sqrt(var)
 *   CONST:  f = alpha                          (applies where sa > 0 and sa is finite)
 *   RTPS:   sb = the saved spread at the point (applies where sa > 0, sa finite and sb finite)
 *           t = sb - sa;  r = t / sa;  g = alpha * r;  f = 1.0 + g
 *   where the rule applies and f != 1.0:  p = f * d_m;  x_m = mean + p  for every m
 * Everywhere else the point is not written and its recorded factor is 1.0: land, where every member holds
 * the same value (sa = 0); a point where any member holds NaN or Inf (sa is NaN); f exactly 1.0.  So
 *   alpha = 0 in RTPS and alpha = 1 in CONST leave every bit of every member as it was (RTPS: wherever r is
 *   finite; t / sa overflows only where sa is below sb x 2^-1023, an analysis spread in the denormals under an
 *   O(1) prior spread, and 0 x Inf is then NaN: the rule is applied as written);
 *   a NaN in one member never spreads to the others;
 *   a halo point and the neighbour block's interior point with the same global indices get the same
 *   operations: if they and the saved spreads held the same bits before, they hold the same bits after.
 * The factor applied, or 1.0, is stored at every point of the array in a second buffer the ensemble owns (one
 * per field and block, as above).  One launch per field and block (values in registers up to 32 members in
 * use; beyond, the members are read once per pass: sum, variance, update).  Afterwards each listed field of
 * each member in use counts as UPLOADED, with exactly ocn_ens_transform's bookkeeping.
 *
 * Both asynchronous on the ensemble's stream.  ocn_ens_inflate_download: the whole array of block k of one of
 * the two buffers of real(8) field field_id (PRIOR_SPREAD: the last ocn_ens_spread_save's; FACTOR: the last
 * ocn_ens_inflate's), in ocn_ctx_download's layout; synchronous.
 * OCN_ERR_ARG -- nothing launched, no member's tail, state or bookkeeping touched, the buffers as they were --
 * for a null ensemble, list or host array, nfields < 1, an id that is real(4), absent or repeated, fewer than
 * two members in use, a bad k, an unknown mode or `what`, an alpha that is not finite, RTPS with alpha < 0.
 * OCN_ERR_STATE, likewise with nothing touched, for RTPS on a field with no saved spread or one saved over a
 * different set of members, and for a download of a buffer that was never formed. */
int ocn_ens_spread_save(ocn_ens *ens, const int32_t *field_ids, int32_t nfields, const uint8_t *use);
enum { OCN_ENS_INFLATE_CONST = 0, OCN_ENS_INFLATE_RTPS = 1 };
int ocn_ens_inflate(ocn_ens *ens, const int32_t *field_ids, int32_t nfields, const uint8_t *use,
                    int32_t mode, double alpha);
enum { OCN_ENS_INFLATE_PRIOR_SPREAD = 0, OCN_ENS_INFLATE_FACTOR = 1 };
int ocn_ens_inflate_download(ocn_ens *ens, int32_t k, int32_t field_id, int32_t what, double *host);

/* Correlated random perturbations of the members, drawn on the device: what makes the members of a freshly
 * initialised ensemble differ, and the additive (model-error) inflation that goes with RTPS after each
 * analysis.  ocn_ens_init_state, ocn_ens_perturb, ocn_ens_step, ocn_ens_spread_save, ocn_ens_assimilate,
 * ocn_ens_inflate, ocn_ens_perturb, ocn_ens_step are asynchronous calls on the ensemble's stream with no host
 * wait and no upload.  No counterpart in the reference.
 *
 * The members in use are u0 < u1 < ... < u(n-1) in member order (use as in ocn_ens_stats), n >= 1.  Each
 * listed real(8) field field_ids[f], f < nfields, has a draw id draw[f] and a mask mask_ids[f]: a real(4)
 * field id (OCN_LU, OCN_LCU, OCN_LLU, ...) or -1 for none.  The points are those of every local block's array
 * A(bnd_x1:bnd_x2, bnd_y1:bnd_y2), with the library's 1-based global indices (i, j).  The random part is
 * integer arithmetic, so its result does not depend on any order of evaluation, and a point's perturbation is
 * a function of (seed, draw, member, i, j, reach, passes, n, centre, amplitude) alone: it does not depend on
 * the block decomposition, and a halo point gets what the owning block's interior point gets.
 *   White noise: (o0, o1, o2, o3) = Philox4x32-10 of the counter ((uint32_t)(int32_t)i, (uint32_t)(int32_t)j,
 *     u_m, draw[f]) under the key (seed & 0xffffffff, seed >> 32) -- multipliers 0xD2511F53, 0xCD9E8D57, key
 *     increments 0x9E3779B9, 0xBB67AE85, 10 rounds; u_m is the member's index in the ensemble, not its rank
 *     among those in use.  S = the sum of the eight 16-bit halves of the four words; W_m(i, j) = S - 262140:
 *     an integer of mean 0, |W| < 2^18.  W is defined on the whole index plane: indices outside the basin,
 *     negative ones included, are taken as they are.
 *   Correlation: Z_m = B_y^P B_x^P W_m with (B_x Z)(i, j) = the sum over d = -R .. R of Z(i + d, j), a box
 *     sum, not a mean; R = reach, 0 .. OCN_ENS_PERTURB_MAX_REACH, P = passes, 0 .. OCN_ENS_PERTURB_MAX_PASSES;
 *     R = 0 or P = 0 gives Z = W.  All values int64.  A point's Z depends on W within R P points of it.
 *   Centring (centre != 0): T = the sum of Z_m over the members in use; D_m = n Z_m - T, so that the D_m of a
 *     point sum to 0 exactly.  Without: D_m = Z_m.
 *   Coefficient, on the host, once per call: q = the sum of k_t^2, k the 1-D box of width 2R+1 convolved with
 *     itself P times (the delta for P = 0), an integer; den = kSigma * (double)q; with centring
 *     den = den * (double)n; c = amplitude / den, with kSigma = 0x1.a20bd6fff1bdfp+15 = sqrt(2 (2^32 - 1) / 3),
 *     the standard deviation of S.  `amplitude` is then the standard deviation of the perturbation; with
 *     centring the expectation of the sample variance over the members (n-1 denominator) is amplitude^2.
 *   Update, where the mask applies -- mask_ids[f] < 0, or member 0's mask field > 0.5f at the point -- each
 *     line one IEEE double operation, no contraction:  d = (double)D_m;  p = c * d;  x_m = x_m + p.
 *     Elsewhere the point is not stored to: land keeps its bits, -0.0 included.  A NaN or Inf stays what it
 *     is and reaches no other member.
 * Exactness: the call is refused unless n (2R+1)^(2P) 2^19 <= 2^53, which bounds |D| by 2^53 and makes
 * (double)D exact: all 256 members up to R = 16 with P = 2, 13 members at R = 16 with P = 3.
 * The bookkeeping is ocn_ens_transform's: the pending call tail of every member in use is formed first, a
 * member not in use is not touched, afterwards each listed field of each member in use counts as UPLOADED and
 * nothing else is re-formed.  Z goes through an int64 scratch the ensemble owns (per block, one array per
 * member in the members' layout, allocated at first use, freed by ocn_ens_destroy).  Launches: the distinct
 * draw ids are taken in the order of their first appearance; per draw id and block ONE noise launch forms Z
 * for all members in use, then one launch per field of that draw id applies it -- fields that share a draw
 * id get the same perturbation.  Asynchronous on the ensemble's stream; the caller's arrays may be reused
 * when the call returns.
 * ocn_ens_perturb_download: Z of the a-th member in use (a < n of that call) from the last noise launch on
 * block k -- the last draw id of the last call -- the whole array in ocn_ctx_download's layout, int64;
 * synchronous.
 * OCN_ERR_ARG -- nothing launched, no member's tail, state or bookkeeping touched, the scratch as it was -- for
 * a null argument (use apart), nfields < 1, an id that is real(4), absent or repeated, a mask id that is
 * neither -1 nor a real(4) field, reach or passes out of range, an amplitude that is not finite and > 0,
 * n < 1, centring with n < 2, the exactness bound; for the download a bad k or a, a null host array.
 * OCN_ERR_STATE for a download before the first successful call. */
enum { OCN_ENS_PERTURB_MAX_REACH = 16, OCN_ENS_PERTURB_MAX_PASSES = 3 };
int ocn_ens_perturb(ocn_ens *ens, const int32_t *field_ids, const int32_t *mask_ids, const uint32_t *draw,
                    int32_t nfields, const uint8_t *use, uint64_t seed, int32_t reach, int32_t passes,
                    int32_t centre, double amplitude);
int ocn_ens_perturb_download(ocn_ens *ens, int32_t k, int32_t a, int64_t *host);

/* Moving-storm forcing: the wind stress and the air pressure of a storm that moves across the basin, formed on
 * the device into OCN_RHSX / OCN_RHSY (the external momentum forcing of sw_update_uv) from a few numbers per
 * member, at each step's own time -- a storm-surge ensemble whose members differ in the storm's track, size
 * and strength.  No counterpart in the reference.
 *
 * ocn_ens_storm (one per member): x0, y0 the centre at t = 0 in GLOBAL 1-based index coordinates (fractional);
 * cx, cy index steps per second; radius (m, > 0); vmax (m/s, >= 0); dp (Pa, >= 0) the central pressure deficit;
 * cos_in, sin_in the inflow angle's cosine and sine, formed by the host (the device takes no sin or cos); turn
 * +1.0 or -1.0, the sense of rotation.  ocn_ens_forcing_model (one per ensemble): the densities, the drag
 * cd = min(cd0 + cd1 |U|, cd_max) and a background wind ub, vb.
 *
 * The point function (csrc/ens_forcing_point.h, the one text the device and the CPU test compile; every line one
 * IEEE double operation, -ffp-contract=off, IEEE division and sqrt, exp = csrc/ocn_exp.h exp_libm; real(4)
 * operands promoted first; ocean_model_arch_amd/ens_forcing_rule.py restates it in numpy):
 *   per storm and time t:   p = cx t, xc = x0 + p;  p = cy t, yc = y0 + p;  rr = R R;  sv = vmax / R;
 *                           ra = rho_air / rho_water
 *   offsets of the index position (xi, yj) with sx, sy metres per index step:
 *                           d = xi - xc, ex = d sx;  d = yj - yc, ey = d sy
 *                           a = ex ex, b = ey ey, s = a + b, q = s / rr
 *   wind:                   h = 0.5 q, a = 0.5 - h, a = a > -500 ? a : -500;  e = exp(a), s = sv e
 *                           (a Gaussian vortex: the speed is vmax at r = R; no division by r, no pow, no log)
 *                           te = turn ey, a = te cos_in, a = -a, b = ex sin_in, c = a - b, c = s c, uw = ub + c
 *                           te = turn ex, a = te cos_in,         b = ey sin_in, c = a - b, c = s c, vw = vb + c
 *                           a = uw uw, b = vw vw, s = a + b, w = sqrt(s)
 *                           c = cd1 w, c = cd0 + c, cd = c < cd_max ? c : cd_max;  k = ra cd, k = k w
 *                           taux = k uw, tauy = k vw            (the kinematic stress)
 *   pressure:               h = -0.5 q, h = h > -500 ? h : -500;  e = exp(h), pa = dp e, pa = -pa
 *   RHSx(m, n), the u-point (m + 1/2, n), where lcu(m, n) > 0.5 (else +0.0):
 *                           the wind at (m + 0.5, n) with sx = dxt(m, n), sy = dyh(m, n)
 *                           pa0, pa1 = the pressure at (m, n) and (m + 1, n), each with its own point's dx, dy
 *                           ar = dxt dyh, a = taux ar;  d = pa1 - pa0, d = d / rho_water, d = d dyh
 *                           hu = h_r(m, n) + h_r(m + 1, n), hu = 0.5 hu;  d = d hu;  RHSx = a - d
 *   RHSy(m, n), the v-point (m, n + 1/2), where lcv(m, n) > 0.5 (else +0.0):
 *                           the wind at (m, n + 0.5) with sx = dxh(m, n), sy = dyt(m, n)
 *                           pa0, pa1 = the pressure at (m, n) and (m, n + 1)
 *                           ar = dyt dxh, a = tauy ar;  d = pa1 - pa0, d = d / rho_water, d = d dxh
 *                           hv = h_r(m, n) + h_r(m, n + 1), hv = 0.5 hv;  d = d hv;  RHSy = a - d
 * The pressure term is sw_update_uv's slx / sly with pa / rho_water in the place of g ssh, linearized about the
 * rest depth h_r (OCN_HHQ_REST): nothing a call's tail forms is read.  Both arrays are written at the interior
 * points nx_start..nx_end x ny_start..ny_end only (all the general one-pass variant reads), from global indices:
 * the result does not depend on the block grid.
 *
 * ocn_ens_forcing_check (pure, no device, as ocn_ens_plan): what ocn_ens_forcing_set refuses in n storms and a
 * model -- a null argument, n < 1, a value that is not finite, radius <= 0, vmax, dp, a density, cd0, cd1 or cd_max
 * negative, rho_water = 0, turn neither +1 nor -1, cos_in^2 + sin_in^2 off 1 by more than 1e-12: OCN_ERR_ARG.
 * ocn_ens_forcing_set(ens, use, storms, model): after that check, storms[i] (one entry per member of the
 * ensemble, read where use[i] != 0; use NULL: all) becomes member i's storm and the member is FORCED until
 * ocn_ens_forcing_clear; members not in use keep what they had; the model replaces the ensemble's.  A forced
 * member steps with the general one-pass variant at once (as with OCN_OPT_KNOWN_CONSTANTS 0: no verdict to wait
 * for) and runs no pair launches (OCN_OPT_PAIR 2 would defer steps whose forcing belongs to another time);
 * nothing changes for a context that is not forced.  ocn_ens_forcing_clear: no member is forced any more; the
 * arrays keep the last forcing.
 * ocn_ens_forcing_apply(ens, t): both arrays of every forced member for time t, one launch per local block
 * (k_ens_forcing, csrc/ens_forcing.hip).  The pending call tails of the forced members are formed first (a tail
 * re-runs the last step and must find that step's forcing); afterwards the two fields count as UPLOADED
 * (ocn_ctx_upload's bookkeeping).  Any block grid, with or without tracers.  Asynchronous.
 * ocn_ens_step_forced(ens, tau, nsteps, check_every, t0): nsteps steps of every member, step s (0-based) of a
 * forced member with the forcing of t_s = t0 + (double)s tau; the checks at the steps s + 1 of this call that
 * check_every divides.  Every field of every member afterwards is bit for bit what
 * ocn_ens_forcing_apply(t_s); ocn_ens_step(tau, 1, ...) per step leaves: OCN_RHSX / OCN_RHSY hold the LAST
 * step's forcing, so a later ocn_ens_complete re-runs that step correctly.  Members that are not forced step as
 * in ocn_ens_step.  Asynchronous on the ensemble's stream, no host wait.  Two routes, the same bits:
 *   chunked (always available): that loop.  A forced member whose open sequence the next step goes on with
 *     (ocn_ens_step's lazy call tail: same tau, nothing deferred) has its two arrays rewritten under it with no
 *     tail formed and nothing dropped -- its state is current and the pending tail will be that next step's -- so
 *     its sequence stays open; every other forced member goes through ocn_ens_forcing_apply's bookkeeping.
 *   in the launch (OCN_ENS_OPT_FORCING_IN_LAUNCH 1, the default; 0 for tests and measurements): where every forced
 *     member would go into a multi-step launch group that goes on with its open sequence (what ocn_ens_step batches:
 *     one small block, no tracers, check_every 0 or 1, at least 2 steps -- an earlier ocn_ens_step or
 *     ocn_ens_step_forced call has opened the sequence), the groups that hold a forced member go as forcing
 *     launches (sw_kernels.hip k_march_multi_frc, the general bodies): the forcing of t0 is written by one
 *     k_ens_forcing launch ahead of them, and between the member's barriers each marching workgroup writes its
 *     share of the NEXT step's forcing into the other of two buffers (the arrays themselves and a second pair the
 *     ensemble owns per forced member, made at the first such call).  After an even number of steps the last
 *     step's forcing is in the second pair: one more k_ens_forcing launch behind the groups forms it into the
 *     arrays themselves.  A capacity of its own (the forcing kernels' occupancy) applies to such calls only.
 * OCN_ERR_STATE with no forced member or before ocn_ens_init_state, OCN_ERR_ARG for nsteps < 0 or a tau or t0 that
 * is not finite.
 * ocn_ens_forcing_info: attached = forced members; applies = k_ens_forcing passes so far (ocn_ens_forcing_apply's
 * and ocn_ens_step_forced's); steps = steps ocn_ens_step_forced has run; in_launch = 1 if the last
 * ocn_ens_step_forced took the in-launch route, else 0. */
typedef struct ocn_ens_storm {
    double x0, y0, cx, cy, radius, vmax, dp, cos_in, sin_in, turn;
} ocn_ens_storm;
typedef struct ocn_ens_forcing_model {
    double rho_air, rho_water, cd0, cd1, cd_max, ub, vb;
} ocn_ens_forcing_model;
typedef struct ocn_ens_forcing_info_t {
    int32_t attached, in_launch;
    int64_t applies, steps;
} ocn_ens_forcing_info_t;
int ocn_ens_forcing_check(const ocn_ens_storm *storms, int32_t n, const ocn_ens_forcing_model *model);
int ocn_ens_forcing_set(ocn_ens *ens, const uint8_t *use, const ocn_ens_storm *storms, const ocn_ens_forcing_model *model);
int ocn_ens_forcing_clear(ocn_ens *ens);
int ocn_ens_forcing_apply(ocn_ens *ens, double t);
int ocn_ens_step_forced(ocn_ens *ens, double tau, int32_t nsteps, int32_t check_every, double t0);
int ocn_ens_forcing_info(ocn_ens *ens, ocn_ens_forcing_info_t *out);

/* The peak map: per point and member the highest and / or lowest value a prognostic field has had after a step,
 * and the number of that step, kept on the device between the steps of the ensemble's launches (csrc/ens_peak.hip
 * k_ens_peak, csrc/sw_kernels.hip k_march_multi_pk; the rule is csrc/ens_peak_point.h, its numpy restatement
 * ocean_model_arch_amd/ens_peak_rule.py).
 *
 * ocn_ens_peak_begin(ens, use, field_id, what): field_id one of OCN_SSH, OCN_SSHP, OCN_UBRTR, OCN_UBRTRP, OCN_VBRTR,
 * OCN_VBRTRP (the recorder's set); what a mask of OCN_ENS_PEAK_MAX and OCN_ENS_PEAK_MIN.  For each extreme asked
 * for, every tracked member (use as in ocn_ens_stats: one byte per member, NULL: all) gets per local block an array
 * P of doubles in the members' layout and an array S of int32 with the same element indexing.  Steps that pair
 * launches deferred are run first for the tracked members (no other call tail is formed); then P = the field's
 * current value and S = 0 at every interior point nx_start..nx_end x ny_start..ny_end, land included; everything
 * outside the interior is +0.0 / 0 and is never written again; the step counter k is 0.  A second begin starts
 * over (the new arrays are whole before the earlier ones go).  Asynchronous.
 * The rule: after the k-th step since begin, with x the field's value after that step (what the CPU oracle holds
 * after as many step(tau) calls: the recorder's contract),
 *     MAX:  if (x > P || P != P) { P = x; S = k; }          MIN: the same with <
 * -- ocn_ens_stats' MIN / MAX comparisons: a tie, +-0 included, keeps the earlier step and its bits; a NaN in P goes
 * as soon as a number arrives; a NaN x never replaces a number.
 * Who steps the peaks: ocn_ens_step and ocn_ens_step_forced, after each of their steps, for the tracked members,
 * while a peak is active (without one they take exactly the path they take without this section).  counted + nsteps
 * beyond INT32_MAX is OCN_ERR_ARG.  ocn_ens_step_record with a peak active is OCN_ERR_STATE: recording and peaks
 * in one launch are built through ocn_ens_run (below), which steps both; ocn_ens_step_record itself still
 * refuses.  Entries that change the state without stepping (ocn_ens_transform, the
 * assimilation entries, ocn_ens_inflate, ocn_ens_perturb, ocn_ctx_upload, ocn_ens_init_state) touch neither P, S
 * nor k, and neither does stepping a member's own context (ocn_ctx_step): the peaks then miss those steps.
 * Two routes, decided before any step of the call runs, the same bits:
 *   in the launch (OCN_ENS_OPT_PEAK_IN_LAUNCH 1, the default; 0 for tests and measurements): with nsteps >= 2, one
 *     local block, every tracked member planning ONE multi-step launch that lands in a group under the capacity of
 *     the kernels with the update in them and, for ocn_ens_step_forced, its own in-launch conditions, the groups
 *     that hold a tracked member go as k_march_multi_pk launches: behind the barrier of every step but the last the
 *     marching workgroups update P and S themselves; one k_ens_peak launch behind the groups does the last step's.
 *   chunked: per step the forcing of that step (a forced call), the step as a 1-step call (the checks at the
 *     steps of THIS call that check_every divides), the tracked members' deferred steps, one k_ens_peak launch per
 *     block.
 * Everything runs on the ensemble's stream with no host wait.
 * ocn_ens_peak_info: active, field, what, tracked members, steps counted (k), and in_launch, the steps whose
 * update a marching launch did itself (cumulative since begin).
 * ocn_ens_peak_download(ens, member, k, which, P_host, S_host): member's arrays of block k for which =
 * OCN_ENS_PEAK_MAX or OCN_ENS_PEAK_MIN in ocn_ctx_download's layout (P_host doubles, S_host int32; either may be
 * NULL, not both).  Synchronous.  ocn_ens_peak_end frees the arrays.
 * ocn_ens_peak_stats(ens, k, which, use, stat_bits): ocn_ens_stats over the P arrays of `which` of the members in
 * use (NULL: the tracked ones; otherwise a subset of them) on block k, into the buffers ocn_ens_stats owns: read
 * them with ocn_ens_stats_download / ocn_ens_stats_output_r4.  Asynchronous.
 * ocn_ens_peak_exceed(ens, k, use, threshold, host): per point of block k's array, c = the number of members in
 * use, in member order, with Pmax > threshold (a NaN is not counted), host = (double)c / (double)n in
 * ocn_ctx_download's layout.  One launch, downloaded through pinned memory; synchronous.  OCN_ENS_PEAK_MAX must be
 * tracked; the threshold may be any double but NaN.
 * Errors: OCN_ERR_ARG -- no member's tail, state or bookkeeping touched, no buffer touched, an earlier peak kept --
 * for a null argument, a field outside the six, what or which outside the masks, an extreme that is not tracked,
 * no member in use, a member in use that is not tracked, a bad member or block index, a NaN threshold;
 * OCN_ERR_STATE for every entry except ocn_ens_peak_begin while no peak is active, and for ocn_ens_peak_begin
 * before ocn_ens_init_state. */
enum { OCN_ENS_PEAK_MAX = 1, OCN_ENS_PEAK_MIN = 2 };
enum { OCN_ENS_OPT_PEAK_IN_LAUNCH = 6 /* ocn_ens_set_option: 1 (default) or 0 */ };
typedef struct ocn_ens_peak_info_t {
    int32_t active, field, what, tracked;
    int64_t steps, in_launch;
} ocn_ens_peak_info_t;
int ocn_ens_peak_begin(ocn_ens *ens, const uint8_t *use, int32_t field_id, int32_t what);
int ocn_ens_peak_end(ocn_ens *ens);
int ocn_ens_peak_info(ocn_ens *ens, ocn_ens_peak_info_t *out);
int ocn_ens_peak_download(ocn_ens *ens, int32_t member, int32_t k, int32_t which, double *P_host, int32_t *S_host);
int ocn_ens_peak_stats(ocn_ens *ens, int32_t k, int32_t which, const uint8_t *use, int32_t stat_bits);
int ocn_ens_peak_exceed(ocn_ens *ens, int32_t k, const uint8_t *use, double threshold, double *host);

/* One entry that steps with everything that is active: the forcing (forced != 0: step s of a forced member under
 * the forcing of t0 + (double)s tau; t0 is not read otherwise), the station recorder and the peak map.
 *
 * ocn_ens_run(ens, tau, nsteps, check_every, forced, t0).  The results are the composition of the three contracts
 * above and nothing new numerically:
 *   members   every member ends exactly as after ocn_ens_step_forced(tau, nsteps, check_every, t0) if forced, else
 *             as after ocn_ens_step(tau, nsteps, check_every): the same bits, the same statuses at
 *             ocn_ens_synchronize;
 *   recorder  if one is active the call counts its steps and writes every record that falls due, exactly as
 *             ocn_ens_step_record defines them (ocn_ens_record_due's schedule);
 *   peak      if one is active, P / S of every tracked member follow every step by the rule above and k advances
 *             by nsteps.
 * With no recorder active the call IS ocn_ens_step_forced or ocn_ens_step (peaks included, as they are there);
 * with a recorder, not forced and no peak active, it IS ocn_ens_step_record.  A recorder together with a peak
 * and / or forced is this entry's own ground, in two routes decided before any step of the call runs, the same
 * bits:
 *   in the launch (OCN_ENS_OPT_RUN_IN_LAUNCH 1, the default, and the in-launch option of every feature that is
 *     active; 0 for tests and measurements): with nsteps >= 2, one local block, every member that is recorded,
 *     tracked or forced planning ONE multi-step launch that lands in a group under the least of the capacities
 *     involved, and a forced call's own in-launch conditions for the forced members.  A group that holds a
 *     recorded member and a forced or tracked one goes as one k_march_multi_all launch (csrc/sw_kernels.hip): the
 *     next step's forcing ahead of each member barrier, the peak update and the due records behind it; every other
 *     group goes as the launch it would be in the entry that covers it.  Behind the groups, in this order: the
 *     forcing's home-coming launch (after an even number of steps), one k_ens_peak launch for the last step, one
 *     gather launch if a record is due at the last step.
 *   chunked: per step the forcing of that step (a forced call), the step as a 1-step call (the checks at the steps
 *     of THIS call that check_every divides), the deferred steps of the tracked and recorded members, one
 *     k_ens_peak launch per block if a peak is active, one gather launch if the step is due.
 * The counters move as in the three entries: ocn_ens_record_info's in_launch by the records written inside
 * launches, ocn_ens_peak_info's by nsteps - 1 for an in-launch call, ocn_ens_forcing_info's in_launch = 1 / 0 for
 * a forced call.  Asynchronous on the ensemble's stream, no host wait.
 * OCN_ERR_ARG or OCN_ERR_STATE -- nothing stepped, launched, written or counted -- for a null ensemble, nsteps < 0,
 * a tau (or, forced, a t0) that is not finite, a call whose due records would pass max_records, a peak step count
 * beyond INT32_MAX, forced with no storm attached, a member that is not initialised. */
enum { OCN_ENS_OPT_RUN_IN_LAUNCH = 7 /* ocn_ens_set_option: 1 (default) or 0 */ };
int ocn_ens_run(ocn_ens *ens, double tau, int32_t nsteps, int32_t check_every, int32_t forced, double t0);

const char *ocn_last_error(void);
int ocn_abi_version(void);
/* Build id: a hash of the library's sources and compile flags (Makefile), e.g. to tie a
 * profile taken on one build to the library that is loaded. */
const char *ocn_build_id(void);
/* Kernel launches this process has issued through the library so far (every context, copies
 * between buffers not included): a host takes differences around a region to count launches. */
int64_t ocn_launch_count(void);

/* The two-step launch's tile plan (pure, no device, as ocn_ens_plan; the function the launches themselves
 * call): a range of width x height points is cut into workgroup tiles of 116 columns and *rows rows; a
 * tile's workgroup passes *rows + 8 iterations, the chip holds 512 workgroups of it at once, and `mult`
 * ranges of this size share one launch (a batch of blocks).  The plan is the tile height with the fewest
 * iterations in total, *iterations = *rounds x (*rows + 8), among 8 .. 150 rows (what the workgroup's LDS
 * table of row constants holds); the smallest such height is taken.  nv != 0 asks for the plan of the
 * inviscid bodies (OCN_OPT_INVISCID): today the same one, they share the cap.  A fixed height
 * (ocn_set_pair_rows) replaces the search, clipped to the cap.
 * OCN_ERR_ARG for a size or mult below 1 or a null output pointer. */
int ocn_pair_plan(int width, int height, int mult, int nv, int *rows, int *rounds, int *iterations);
/* A fixed tile height for every two-step launch of the process from now on, clipped to the cap of 150
 * rows; 0 = automatic (ocn_pair_plan's search).  The environment variable OCN_PAIR_ROWS, read when
 * the library is loaded, is its initial value (a value below 8 there counts as 0).  A tuning and testing
 * aid, not a context option: it takes effect for launches issued after the call, and a step captured as a
 * graph is captured again under a new height.  OCN_ERR_ARG for a negative value or 1 .. 7. */
int ocn_set_pair_rows(int rows);

#ifdef __cplusplus
}
#endif
#endif /* OCN_SW_H */
