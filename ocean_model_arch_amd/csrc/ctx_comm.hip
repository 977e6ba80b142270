// ctx_comm.hip -- halo exchange of the model context (ocn_ctx.h): the segment copy kernels, the halo
// plans, the RCCL and loopback transports, the role-flip vote's reduction, run_sync, and the host-side
// watchdog of the entries that may take part in a collective.
//
// Reference counterparts (Andrcraft9/ocean_model_arch):
//   halo           shared/mpp/sync.f90:294-556 + syncborder_block2D_gen_all.fi
//   neighbour maps core/decomposition.f90:950-1062
#include "ocn_ctx.h"

namespace ocn {

// ------------------------------------------------------------------ halo segments (ocn_ctx.h Seg)
// Grid: one workgroup per 64-element chunk of a segment (SegChunk: the chunk table of the list, so
// no workgroup of a short segment idles as in a segments x longest-chunks grid); element e of a
// segment: run j = e % w, row i = e / w -- one element per thread and one wave per workgroup, so
// every load of a strip is in flight at once, spread over many CUs (a loop per workgroup would pay
// one memory round trip per pass).
constexpr int kSegChunk = 64;
__device__ __forceinline__ bool seg_at(const Seg &g, int e, long &si, long &di)
{
    if (e >= g.count * g.w) return false;
    const int i = e / g.w, j = e - i * g.w;
    si = (long)i * g.src_stride + (long)j * g.src_jstride;
    di = (long)i * g.dst_stride + (long)j * g.dst_jstride;
    return true;
}
__global__ __launch_bounds__(kSegChunk) void k_segments(const Seg *__restrict__ segs, const SegChunk *__restrict__ ch,
                                                        int nch)
{
    const int b = blockIdx.x;
    if (b >= nch) return;
    const SegChunk q = ch[b];
    const Seg g = segs[q.seg];
    long si, di;
    if (!seg_at(g, q.e0 + (int)threadIdx.x, si, di)) return;
    g.dst[di] = g.src[si];
}

// The same runs compared instead of copied: ORs 1 into *flags where dst differs from src (bits).
__global__ __launch_bounds__(kSegChunk) void k_segments_cmp(const Seg *__restrict__ segs, const SegChunk *__restrict__ ch,
                                                            int nch, int32_t *flags)
{
    const int k = blockIdx.x;
    if (k >= nch) return;
    const SegChunk q = ch[k];
    const Seg g = segs[q.seg];
    long si, di;
    if (!seg_at(g, q.e0 + (int)threadIdx.x, si, di)) return;
    const double a = g.dst[di], b = g.src[si];
    unsigned long long x, y;
    __builtin_memcpy(&x, &a, 8);
    __builtin_memcpy(&y, &b, 8);
    if (x != y) atomicOr(flags, 1);
}

// Strip of a Rect inside a block array as (offset, count, stride): a 1-wide rect is a row
// (stride 1) or a column (stride pitch).
static void strip(const ocn_block &b, const Rect &r, long &off, int &count, long &stride)
{
    off = (long)(r.x0 - b.bnd_x1) + (long)(r.y0 - b.bnd_y1) * (long)b.pitch;
    if (r.y0 == r.y1) { count = r.x1 - r.x0 + 1; stride = 1; }
    else { count = r.y1 - r.y0 + 1; stride = (long)b.pitch; }
}

// v on the device with its chunk table (one entry per kSegChunk elements of each segment), in one
// allocation freed with the context
int make_seglist(ocn_ctx *c, const std::vector<Seg> &v, SegList &out)
{
    out = SegList{};
    std::vector<SegChunk> ch;
    for (size_t i = 0; i < v.size(); ++i)
        for (long e = 0; e < (long)v[i].count * v[i].w; e += kSegChunk) ch.push_back(SegChunk{(int)i, (int)e});
    if (v.empty() || ch.empty()) return OCN_OK;
    const size_t sb = sizeof(Seg) * v.size(), cb = sizeof(SegChunk) * ch.size();
    char *d = nullptr;
    HIPCHK(hipMalloc(&d, sb + cb));
    c->allocs.push_back(d);
    HIPCHK(hipMemcpy(d, v.data(), sb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + sb, ch.data(), cb, hipMemcpyHostToDevice));
    out.d = (Seg *)d;
    out.ch = (SegChunk *)(d + sb);
    out.n = (int)v.size();
    out.nch = (int)ch.size();
    return OCN_OK;
}
// the list's copies on s (cmp: compared instead, 1 ORed into *cmp where they differ)
int launch_segs(const SegList &l, hipStream_t s, int32_t *cmp)
{
    if (!l.nch) return OCN_OK;
    if (cmp) hipLaunchKernelGGL(k_segments_cmp, dim3((unsigned)l.nch), dim3(kSegChunk), 0, s, l.d, l.ch, l.nch, cmp);
    else hipLaunchKernelGGL(k_segments, dim3((unsigned)l.nch), dim3(kSegChunk), 0, s, l.d, l.ch, l.nch);
    return check_launch();
}

// ------------------------------------------------------------------ halo plans
// syncborder_block2D_gen_all.fi: halo of block k in dir d <- boundary of neighbour in inverse(d).
// Messages between two processes carry, for every (sending block, dir) pair in global block
// order and every field of the sync group, the boundary strip in column-major order.
// Host-only schedule of one halo exchange (no device pointers): every entry copies the
// 1-wide strip `src` of local block ks (local copy or send) into the strip `dst` of local block
// k (local copy or receive).  Message layout between two processes: for every (receiving
// block, dir) in global block order, every field of the group, the sender's boundary strip in
// column-major order -- enumerated identically on both sides from global knowledge.
struct PlanEntry {
    int kind;          // OCN_HALO_LOCAL / OCN_HALO_SEND / OCN_HALO_RECV
    int peer;          // rank (send/recv), own rank for local
    int k, ks;         // destination / source local block (-1 where not applicable)
    int field;
    Rect dst, src;
    long buf_off;      // element offset in the peer's message (send/recv)
    int count;
};

// Layer j (1 .. depth) of the halo of block `rcv` in direction d and the boundary of its
// neighbour `src` it receives: layer 1 is the reference's 1-wide exchange (syncborder_block2D_gen_all.fi);
// layer 2 (depth 2, the one-pass steps' state exchange, one_step_x2) the next row / column out
// (and depth x depth corner patches).  Corner layers are rows of `depth` points.
static void halo_layer(const ocn_block &rcv, const ocn_block &src, int d, int j, int depth, Rect &hr, Rect &br)
{
    const int dm = kDirDm[d], dn = kDirDn[d];
    // x: halo columns / source columns of this direction
    int hx0, hx1, sx0, sx1;
    if (dm > 0) { hx0 = rcv.nx_end + 1; hx1 = rcv.nx_end + (dn ? depth : 1); sx0 = src.nx_start; sx1 = sx0 + (hx1 - hx0); }
    else if (dm < 0) { hx1 = rcv.nx_start - 1; hx0 = rcv.nx_start - (dn ? depth : 1); sx1 = src.nx_end; sx0 = sx1 - (hx1 - hx0); }
    else { hx0 = rcv.nx_start; hx1 = rcv.nx_end; sx0 = src.nx_start; sx1 = src.nx_end; }
    if (dm && !dn) {   // E / W edge: layer j is one column
        hx0 = hx1 = dm > 0 ? rcv.nx_end + j : rcv.nx_start - j;
        sx0 = sx1 = dm > 0 ? src.nx_start + j - 1 : src.nx_end - j + 1;
    }
    int hy, sy;
    if (dn > 0) { hy = rcv.ny_end + j; sy = src.ny_start + j - 1; }
    else if (dn < 0) { hy = rcv.ny_start - j; sy = src.ny_end - j + 1; }
    else { hy = -1; sy = -1; }
    if (dn) { hr = {hx0, hx1, hy, hy}; br = {sx0, sx1, sy, sy}; }
    else { hr = {hx0, hx1, rcv.ny_start, rcv.ny_end}; br = {sx0, sx1, src.ny_start, src.ny_end}; }
}

// Depth of field id in an exchange of `depth`: the tracer fields are exchanged one point deep in
// every exchange (one_step_x2 sends them with the state's two-deep strips: one message per peer)
// tracers: 1 deep, 2 with the x4 pairs' 4-deep state (one_step_x4's first tracer step covers the halo
// ring neighbours own)
static int field_depth(int id, int depth) { return is_tracer_field(id) ? (depth >= 4 ? 2 : 1) : depth; }

static int plan_entries(const ocn_ctx *c, const std::vector<int> &fields, std::vector<PlanEntry> &out,
                        int depth = 1)
{
    out.clear();
    std::map<int, int> k_of_gid;
    for (size_t k = 0; k < c->blocks.size(); ++k) k_of_gid[c->blocks[k].gid] = (int)k;
    std::map<int, long> send_count, recv_count;
    // receiving side: my halos in gid order, dirs 1..8, layers 1..depth
    for (auto &kv : k_of_gid) {
        const int k = kv.second;
        const LBlock &b = c->blocks[k];
        for (int d = 1; d <= 8; ++d) {
            const int r = b.nbr_rank[d - 1];
            if (r < 0) continue;
            const GBlock &src = c->gblocks[b.nbr_gid[d - 1]];
            for (int j = 1; j <= depth; ++j) {
                for (int id : fields) {
                    const int fd = field_depth(id, depth);
                    if (j > fd) continue;
                    Rect hr, br;
                    halo_layer(b.g, src.g, d, j, fd, hr, br);
                    const int cnt = (hr.x1 - hr.x0 + 1) * (hr.y1 - hr.y0 + 1);
                    if (r == c->dec.rank)
                        out.push_back(PlanEntry{OCN_HALO_LOCAL, r, k, k_of_gid.at(b.nbr_gid[d - 1]), id, hr, br, 0, cnt});
                    else {
                        out.push_back(PlanEntry{OCN_HALO_RECV, r, k, -1, id, hr, br, recv_count[r], cnt});
                        recv_count[r] += cnt;
                    }
                }
            }
        }
    }
    // sending side: remote receivers in gid order, dirs 1..8, layers 1..depth, whose source block is mine
    for (size_t gid = 0; gid < c->gblocks.size(); ++gid) {
        const GBlock &rb = c->gblocks[gid];
        if (rb.rank < 0 || rb.rank == c->dec.rank) continue;
        for (int d = 1; d <= 8; ++d) {
            const int m = rb.bm + kDirDm[d], n = rb.bn + kDirDn[d];
            if (m < 1 || m > c->bnx || n < 1 || n > c->bny) continue;
            const int sg = (m - 1) + (n - 1) * c->bnx;
            if (c->gblocks[sg].rank != c->dec.rank) continue;
            const int ks = k_of_gid.at(sg);
            for (int j = 1; j <= depth; ++j) {
                for (int id : fields) {
                    const int fd = field_depth(id, depth);
                    if (j > fd) continue;
                    Rect hr, br;
                    halo_layer(rb.g, c->blocks[ks].g, d, j, fd, hr, br);
                    const int cnt = (br.x1 - br.x0 + 1) * (br.y1 - br.y0 + 1);
                    out.push_back(PlanEntry{OCN_HALO_SEND, rb.rank, -1, ks, id, hr, br, send_count[rb.rank], cnt});
                    send_count[rb.rank] += cnt;
                }
            }
        }
    }
    for (auto &kv : recv_count)
        if (send_count[kv.first] != kv.second) return set_error(OCN_ERR_STATE, "halo plan: asymmetric message sizes");
    for (auto &kv : send_count)
        if (recv_count[kv.first] != kv.second) return set_error(OCN_ERR_STATE, "halo plan: asymmetric message sizes");
    return OCN_OK;
}

// Column strips (a side with a stride) of the same length whose runs are adjacent columns on a strided
// side (step +1 or -1), the other side's runs equally spaced -- as the layers of one field's E / W strip
// are: one segment of w runs (up to kSegMaxW) instead of w, copying the same elements.
constexpr int kSegMaxW = 8;
static std::vector<Seg> merge_columns(const std::vector<Seg> &in)
{
    std::vector<Seg> out;
    std::vector<char> used(in.size(), 0);
    std::map<const double *, size_t> by_src, by_dst;   // the column strips by their strided side
    for (size_t i = 0; i < in.size(); ++i) {
        if (in[i].w != 1) continue;
        if (in[i].src_stride > 1) by_src[in[i].src] = i;
        else if (in[i].dst_stride > 1) by_dst[in[i].dst] = i;
    }
    for (size_t i = 0; i < in.size(); ++i) {
        if (used[i]) continue;
        used[i] = 1;
        Seg g = in[i];
        const bool sc = g.src_stride > 1, dc = !sc && g.dst_stride > 1;
        if (g.w == 1 && (sc || dc)) {
            for (const long step : {1L, -1L}) {
                if (g.w > 1) break;
                while (g.w < kSegMaxW) {
                    auto &idx = sc ? by_src : by_dst;
                    auto it = idx.find((sc ? (const double *)g.src : (const double *)g.dst) + (long)g.w * step);
                    if (it == idx.end() || used[it->second]) break;
                    const Seg &b = in[it->second];
                    if (b.count != g.count || b.src_stride != g.src_stride || b.dst_stride != g.dst_stride) break;
                    // the other side's spacing: set by the second run, kept by the rest
                    const long other = sc ? (long)(b.dst - g.dst) : (long)(b.src - g.src);
                    if (g.w == 1) {
                        if (sc) { g.src_jstride = step; g.dst_jstride = other; }
                        else { g.dst_jstride = step; g.src_jstride = other; }
                    } else if (other != (long)g.w * (sc ? g.dst_jstride : g.src_jstride)) {
                        break;
                    }
                    used[it->second] = 1;
                    ++g.w;
                }
            }
        }
        out.push_back(g);
    }
    return out;
}

static int build_plan(ocn_ctx *c, const std::vector<int> &fields, HaloPlan &plan, int depth = 1)
{
    std::vector<PlanEntry> entries;
    RC(plan_entries(c, fields, entries, depth));
    std::map<int, long> msg;                       // peer -> message length
    for (const PlanEntry &e : entries)
        if (e.kind == OCN_HALO_RECV) msg[e.peer] = std::max(msg[e.peer], e.buf_off + e.count);
    std::map<int, HaloPlan::Peer> peers;
    for (auto &kv : msg) {
        HaloPlan::Peer p{kv.first, kv.second, nullptr, nullptr};
        HIPCHK(hipMalloc(&p.send, sizeof(double) * std::max(1L, p.count)));
        HIPCHK(hipMalloc(&p.recv, sizeof(double) * std::max(1L, p.count)));
        c->allocs.push_back(p.send); c->allocs.push_back(p.recv);
        peers[kv.first] = p;
        plan.peers.push_back(p);
    }
    std::vector<Seg> local, pack, unpack;
    for (const PlanEntry &e : entries) {
        long doff, soff, dstr, sstr; int dcnt, scnt;
        if (e.kind == OCN_HALO_LOCAL) {
            const LBlock &db = c->blocks[e.k], &sb = c->blocks[e.ks];
            strip(db.g, e.dst, doff, dcnt, dstr);
            strip(sb.g, e.src, soff, scnt, sstr);
            local.push_back(Seg{sb.f<double>(e.field) + soff, db.f<double>(e.field) + doff, sstr, dstr, dcnt});
        } else if (e.kind == OCN_HALO_RECV) {
            const LBlock &db = c->blocks[e.k];
            strip(db.g, e.dst, doff, dcnt, dstr);
            unpack.push_back(Seg{peers.at(e.peer).recv + e.buf_off, db.f<double>(e.field) + doff, 1, dstr, dcnt});
        } else {
            const LBlock &sb = c->blocks[e.ks];
            strip(sb.g, e.src, soff, scnt, sstr);
            pack.push_back(Seg{sb.f<double>(e.field) + soff, peers.at(e.peer).send + e.buf_off, sstr, 1, scnt});
        }
    }
    RC(make_seglist(c, merge_columns(local), plan.local));
    RC(make_seglist(c, merge_columns(pack), plan.pack));
    RC(make_seglist(c, merge_columns(unpack), plan.unpack));
    return OCN_OK;
}

// Plans hold raw field pointers, so a plan is kept per role of the buffers its fields swap
// between (the key is the field list followed by -1 - the relevant role bits).
// depth 2: the one-pass steps' 2-deep state exchange (halo_layer); priv: a plan over a private
// buffer swapped into the field table while it is built and run (one_step_x2's h_r copy)
int get_plan(ocn_ctx *c, const std::vector<int> &fields, HaloPlan *&out, int depth, int priv)
{
    std::vector<int> key = fields;
    // a plan holds the buffers its fields had when it was built: the pair roles (bit 1), and for
    // sshp / ubrtrp / vbrtrp the second buffers' roles (bit 4: they persist between one-pass calls)
    const bool alt = std::any_of(fields.begin(), fields.end(), [](int id) { return is_alt_field(id); });
    // (tracer fields: the tracer steps' role bits 8 -- ff1 / ff1n -- and 16 -- ff1p's second buffer)
    const bool tr = std::any_of(fields.begin(), fields.end(), [](int id) { return is_tracer_field(id); });
    key.push_back(-1 - (c->role & 1) - (alt ? (c->role & 4) : 0) - (tr ? (c->role & 24) : 0));
    if (depth != 1 || priv) key.push_back(-100 - depth - 10 * priv);
    auto it = c->plans.find(key);
    if (it == c->plans.end()) {
        if (c->capturing) return set_error(OCN_ERR_STATE, "halo plan built while a step is captured");
        HaloPlan p;
        RC(build_plan(c, fields, p, depth));
        it = c->plans.emplace(key, p).first;
    }
    out = &it->second;
    return OCN_OK;
}

int nccl_rc(ncclResult_t r, const char *what)
{
    if (r == ncclSuccess) return OCN_OK;
    return set_error(OCN_ERR_COMM, std::string(what) + ": " + ncclGetErrorString(r));
}

static int comm_gone(const ocn_ctx *c)
{
    return set_error(OCN_ERR_COMM, "the RCCL communicator was aborted after an earlier fatal error");
}

// a rank of a loopback group that fails releases its peers' waits at once
static int lb_fail_on_error(ocn_ctx *c, int rc)
{
    if (rc && c->lb) {
        std::lock_guard<std::mutex> g(c->lb->mu);
        c->lb->failed = true;
        c->lb->cv.notify_all();
    }
    return rc;
}

// An error inside a call that takes part in collectives (step, init_state, synchronize): the
// loopback group's waits are released (lb_fail_on_error), and a fatal one (HIP, RCCL, state) aborts
// the RCCL communicator -- its queued sends / receives are cancelled and nothing of this rank waits
// on a peer that will not come; the host then ends the job, as abort_model's mpi_abort does
// (shared/errors.f90:30-37).  OCN_ERR_BLOWUP is not fatal here: every rank returns it from the same
// synchronize (sync_impl reduces the counts), and OCN_ERR_ARG is raised before any collective.
int fail_fatal(ocn_ctx *c, int rc)
{
    rc = lb_fail_on_error(c, rc);
    if ((rc && rc != OCN_ERR_BLOWUP && rc != OCN_ERR_ARG) || c->wd_fired.load()) {
        std::lock_guard<std::mutex> g(c->comm_mu);
        if (c->comm) {
            if (!c->comm_abort_done) (void)ncclCommAbort(c->comm);   // (the watchdog may have)
            c->comm_abort_done = true;
            c->comm = nullptr;
            c->comm_aborted = true;
        }
    }
    return rc;
}

// ------------------------------------------------------------------ host-side watchdog
// ocn_ctx_set_watchdog: a thread per context watches the entries that may take part in a collective
// (guarded below).  One that has not returned after wd_s is ended: the message names the call and the
// last exchange with remote peers the device completed (polled from c->xq), the RCCL communicator is
// aborted (RCCL's kernels waiting on a peer exit, so the call's stream wait returns) or the loopback
// group failed (its rendezvous return), and the call returns OCN_ERR_COMM with the message.  A call
// still stuck 10 s later ends the process (exit status 3).
int64_t poll_xdone(ocn_ctx *c)
{
    std::lock_guard<std::mutex> g(c->xmu);
    while (!c->xq.empty() && hipEventQuery(c->xq.front().second) == hipSuccess) {
        c->xdone = c->xq.front().first;
        c->xpool.push_back(c->xq.front().second);
        c->xq.pop_front();
    }
    return c->xdone;
}

static void wd_fire(ocn_ctx *c, const char *call, double waited)
{
    const int64_t done = poll_xdone(c);
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "ocn watchdog: rank %d of %d: %s has not returned after %.1f s (limit %.1f s); last completed "
                  "exchange id %lld of %lld enqueued; %s",
                  c->dec.rank, c->dec.nranks, call, waited, c->wd_s, (long long)done, (long long)c->xchg,
                  c->lb ? "failing the loopback group" : c->comm ? "aborting the RCCL communicator" : "no communicator");
    c->wd_msg = buf;
    c->wd_fired.store(true);
    std::fprintf(stderr, "%s\n", buf);
    std::fflush(stderr);
    if (c->lb) {
        std::lock_guard<std::mutex> g(c->lb->mu);
        c->lb->failed = true;
        c->lb->cv.notify_all();
    }
    std::lock_guard<std::mutex> g(c->comm_mu);
    if (c->comm && !c->comm_abort_done) {
        (void)ncclCommAbort(c->comm);
        c->comm_abort_done = true;
    }
}

void wd_loop(ocn_ctx *c)
{
    (void)hipSetDevice(c->dec.device);
    std::unique_lock<std::mutex> g(c->wd_mu);
    while (!c->wd_stop) {
        c->wd_cv.wait_for(g, std::chrono::milliseconds(100));
        if (c->wd_stop || c->call_depth == 0 || c->wd_fired.load() || c->wd_s <= 0) continue;
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - c->call_t0).count();
        if (waited < c->wd_s) continue;
        const char *call = c->call_name;
        g.unlock();
        wd_fire(c, call, waited);
        g.lock();
        if (!c->wd_cv.wait_for(g, std::chrono::seconds(10), [c] { return c->wd_stop || c->call_depth == 0; })) {
            std::fprintf(stderr, "ocn watchdog: rank %d: %s still blocked 10 s after the abort; exiting (status 3)\n",
                         c->dec.rank, call);
            std::fflush(stderr);
            std::_Exit(3);
        }
    }
}

// An entry that may take part in a collective, watched while a watchdog is set (ocn_ctx.h guarded)
CallGuard::CallGuard(ocn_ctx *ctx, const char *name) : c(ctx)
{
    std::lock_guard<std::mutex> g(c->wd_mu);
    if (c->call_depth++ == 0) {
        c->call_t0 = std::chrono::steady_clock::now();
        c->call_name = name;
    }
}
CallGuard::~CallGuard()
{
    std::lock_guard<std::mutex> g(c->wd_mu);
    --c->call_depth;
    c->wd_cv.notify_all();
}

// One loopback rendezvous: this rank passes phase `ph`, then waits until every rank in `peers`
// has passed it as often (bounded wait: a rank that failed or never comes ends it with an error).
static int lb_meet(ocn_ctx *c, int ph, const std::vector<int> &peers)
{
    Loopback &L = *c->lb;
    const int r = c->dec.rank;
    std::unique_lock<std::mutex> g(L.mu);
    const uint64_t mine = ++L.cnt[ph][r];
    L.cv.notify_all();
    bool lost = false;   // a peer still needed failed or was destroyed
    const bool ok = L.cv.wait_for(g, std::chrono::seconds(120), [&] {
        bool all = true;
        for (int p : peers)
            if (L.cnt[ph][p] < mine) {
                all = false;
                lost = lost || L.failed || !L.ctx[p];
            }
        return all || lost;
    });
    if (!ok || lost) {
        L.failed = true;
        L.cv.notify_all();
        return set_error(OCN_ERR_COMM, "loopback transport: a peer rank did not reach the exchange");
    }
    return OCN_OK;
}

// The ncclRecv / ncclSend pairs of one exchange over the loopback transport (see Loopback).
static int lb_exchange(ocn_ctx *c, const HaloPlan *p, hipStream_t stream)
{
    Loopback &L = *c->lb;
    const int r = c->dec.rank;
    std::vector<int> peers;
    for (const auto &q : p->peers) peers.push_back(q.rank);
    HIPCHK(hipEventRecord(c->lb_ev_a, stream));
    {
        std::lock_guard<std::mutex> g(L.mu);
        L.plan[r] = p;
    }
    RC(lb_meet(c, 0, peers));
    for (const auto &q : p->peers) {
        const HaloPlan *pp;
        hipEvent_t ev;
        {   // a peer destroyed after the rendezvous has left its slot empty: fail, do not dereference
            std::lock_guard<std::mutex> g(L.mu);
            if (!L.ctx[q.rank]) return set_error(OCN_ERR_COMM, "loopback transport: a peer rank was destroyed");
            pp = L.plan[q.rank];
            ev = L.ctx[q.rank]->lb_ev_a;
        }
        const HaloPlan::Peer *src = nullptr;
        for (const auto &e : pp->peers)
            if (e.rank == r) src = &e;
        if (!src || src->count != q.count) return set_error(OCN_ERR_STATE, "loopback transport: message sizes disagree");
        HIPCHK(hipStreamWaitEvent(stream, ev, 0));
        HIPCHK(hipMemcpyAsync(q.recv, src->send, sizeof(double) * (size_t)q.count, hipMemcpyDeviceToDevice, stream));
    }
    HIPCHK(hipEventRecord(c->lb_ev_b, stream));
    RC(lb_meet(c, 1, peers));
    std::vector<hipEvent_t> evs;
    {
        std::lock_guard<std::mutex> g(L.mu);
        for (const auto &q : p->peers) {
            if (!L.ctx[q.rank]) return set_error(OCN_ERR_COMM, "loopback transport: a peer rank was destroyed");
            evs.push_back(L.ctx[q.rank]->lb_ev_b);
        }
    }
    for (hipEvent_t e : evs) HIPCHK(hipStreamWaitEvent(stream, e, 0));
    return OCN_OK;
}

// max over the ranks of one device int32 (the role-flip vote): ncclAllReduce, or over the
// loopback transport every rank reads every rank's word (after its lb_ev_a) into d_red and copies
// it back after all ranks have read (lb_ev_b).
struct VotePtrs { const int32_t *p[64]; int n, words; };
__global__ void k_vote_max(VotePtrs v, int32_t *out)
{
    const int w = (int)threadIdx.x;
    if (w >= v.words) return;
    int32_t m = v.p[0][w];
    for (int i = 1; i < v.n; ++i) m = max(m, v.p[i][w]);
    out[w] = m;
}
int allreduce_max(ocn_ctx *c, int32_t *word, hipStream_t s, int words)
{
    if (c->comm_aborted) return comm_gone(c);
    if (c->wd_fired.load()) return set_error(OCN_ERR_COMM, c->wd_msg);
    if (c->comm)
        return nccl_rc(ncclAllReduce(word, word, (size_t)words, ncclInt32, ncclMax, c->comm, s), "ncclAllReduce");
    if (!c->lb) return OCN_OK;
    Loopback &L = *c->lb;
    std::vector<int> all(L.n);
    for (int i = 0; i < L.n; ++i) all[i] = i;
    HIPCHK(hipEventRecord(c->lb_ev_a, s));
    {
        std::lock_guard<std::mutex> g(L.mu);
        L.vote[c->dec.rank] = word;
    }
    RC(lb_meet(c, 2, all));
    VotePtrs v{};
    v.n = L.n;
    v.words = words;
    std::vector<hipEvent_t> evs;
    {   // snapshot under the lock: a peer destroyed after the rendezvous fails the vote
        std::lock_guard<std::mutex> g(L.mu);
        for (int i = 0; i < L.n; ++i) {
            if (!L.ctx[i]) return set_error(OCN_ERR_COMM, "loopback transport: a peer rank was destroyed");
            v.p[i] = L.vote[i];
            evs.push_back(L.ctx[i]->lb_ev_a);
        }
    }
    for (hipEvent_t e : evs) HIPCHK(hipStreamWaitEvent(s, e, 0));
    int32_t *red = c->d_red;
    hipLaunchKernelGGL(k_vote_max, dim3(1), dim3(64), 0, s, v, red);
    RC(check_launch());
    HIPCHK(hipEventRecord(c->lb_ev_b, s));
    RC(lb_meet(c, 3, all));
    evs.clear();
    {
        std::lock_guard<std::mutex> g(L.mu);
        for (int i = 0; i < L.n; ++i) {
            if (!L.ctx[i]) return set_error(OCN_ERR_COMM, "loopback transport: a peer rank was destroyed");
            evs.push_back(L.ctx[i]->lb_ev_b);
        }
    }
    for (hipEvent_t e : evs) HIPCHK(hipStreamWaitEvent(s, e, 0));
    HIPCHK(hipMemcpyAsync(word, red, sizeof(int32_t) * (size_t)words, hipMemcpyDeviceToDevice, s));
    return OCN_OK;
}

// The end of an exchange with remote peers on `stream`: its timer record, and while a watchdog is set
// an event the watchdog polls for the last completed exchange (c->xq; completed events are recycled)
static int exchange_done(ocn_ctx *c, ocn_ctx::Rec &xrec, hipStream_t stream)
{
    if (c->capturing) return OCN_OK;
    if (xrec.b) {
        HIPCHK(hipEventRecord(xrec.b, stream));
        c->recs.push_back(xrec);
    }
    if (c->wd_s <= 0) return OCN_OK;
    std::lock_guard<std::mutex> g(c->xmu);
    while (!c->xq.empty() && (c->xq.size() > 256 || hipEventQuery(c->xq.front().second) == hipSuccess)) {
        if (hipEventQuery(c->xq.front().second) == hipSuccess) c->xdone = c->xq.front().first;
        else HIPCHK(hipEventSynchronize(c->xq.front().second));   // (256 in flight: the oldest has to finish)
        c->xpool.push_back(c->xq.front().second);
        c->xq.pop_front();
    }
    hipEvent_t e;
    if (!c->xpool.empty()) { e = c->xpool.back(); c->xpool.pop_back(); }
    else HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(hipEventRecord(e, stream));
    c->xq.emplace_back(c->xchg, e);
    return OCN_OK;
}

// cmp != nullptr: compare the halos with what the exchange would deliver instead of writing them
// (ORs 1 into *cmp where they differ); same messages, so every rank must take part.
// OCN_OPT_XCHG_DELAY (tests): one wave waits c->xdelay_us on the device clock (a slow link's latency,
// in front of an exchange with remote peers); the loop always ends
__global__ void k_delay(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
static int launch_delay(ocn_ctx *c, hipStream_t s)
{
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->dec.device));
    const unsigned long long ticks = (unsigned long long)c->xdelay_us * (unsigned long long)(khz > 0 ? khz : 100000) / 1000ull;
    hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, s, ticks);
    return check_launch();
}

int run_sync(ocn_ctx *c, const std::vector<int> &fields, hipStream_t stream, int32_t *cmp, int depth, int priv)
{
    HaloPlan *p;
    RC(get_plan(c, fields, p, depth, priv));
    if (!stream) stream = c->stream;
    ocn_ctx::Rec xrec{OCN_TIMER_EXCHANGE, nullptr, nullptr};
    const bool remote = !p->peers.empty();
    if (remote) {
        if (!has_comm(c)) return set_error(OCN_ERR_COMM, "remote neighbours but no RCCL communicator attached");
        if (c->comm_aborted) return comm_gone(c);
        if (c->wd_fired.load()) return set_error(OCN_ERR_COMM, c->wd_msg);
        if (c->stage_timing && !c->capturing) {   // the exchange on its stream: pack, group, unpack
            RC(get_event(c, xrec.a)); RC(get_event(c, xrec.b));
            HIPCHK(hipEventRecord(xrec.a, stream));
        }
        ++c->xchg;
        if (c->xdelay_us > 0) RC(launch_delay(c, stream));
        RC(launch_segs(p->pack, stream));
        if (c->lb) {
            RC(lb_exchange(c, p, stream));
        } else {
            RC(nccl_rc(ncclGroupStart(), "ncclGroupStart"));
            for (auto &peer : p->peers) {
                RC(nccl_rc(ncclRecv(peer.recv, (size_t)peer.count, ncclDouble, peer.rank, c->comm, stream), "ncclRecv"));
                RC(nccl_rc(ncclSend(peer.send, (size_t)peer.count, ncclDouble, peer.rank, c->comm, stream), "ncclSend"));
            }
            RC(nccl_rc(ncclGroupEnd(), "ncclGroupEnd"));
        }
    }
    if (cmp) {
        RC(launch_segs(p->local, stream, cmp));
        RC(launch_segs(p->unpack, stream, cmp));
        return remote ? exchange_done(c, xrec, stream) : OCN_OK;
    }
    RC(launch_segs(p->local, stream));
    RC(launch_segs(p->unpack, stream));
    if (remote) RC(exchange_done(c, xrec, stream));
    return OCN_OK;
}

}  // namespace ocn

extern "C" {

int ocn_halo_schedule_deep(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask, const int32_t *field_ids,
                           int32_t nfields, int32_t depth, ocn_halo_msg *out, int32_t cap, int32_t *count)
{
    if (!field_ids || nfields < 1) return set_error(OCN_ERR_ARG, "no fields");
    if (depth != 1 && depth != 2 && depth != 4) return set_error(OCN_ERR_ARG, "halo exchanges are 1, 2 or 4 points deep");
    std::vector<int> fields(field_ids, field_ids + nfields);
    for (int id : fields)
        if (id < OCN_SSH || id >= OCN_TRACER_BASE + 3 * kMaxTracers)
            return set_error(OCN_ERR_ARG, "halo exchange is defined for real(8) fields");
    ocn_ctx *c = nullptr;
    RC(host_ctx(basin, dec, mask, c));
    std::vector<PlanEntry> es;
    const int rc = plan_entries(c, fields, es, depth);
    delete c;
    RC(rc);
    if (count) *count = (int32_t)es.size();
    for (size_t i = 0; i < es.size() && (int32_t)i < cap && out; ++i) {
        const PlanEntry &e = es[i];
        ocn_halo_msg &o = out[i];
        o.kind = e.kind; o.peer = e.peer; o.k = e.k; o.k_src = e.ks; o.field = e.field;
        o.dst_x0 = e.dst.x0; o.dst_x1 = e.dst.x1; o.dst_y0 = e.dst.y0; o.dst_y1 = e.dst.y1;
        o.src_x0 = e.src.x0; o.src_x1 = e.src.x1; o.src_y0 = e.src.y0; o.src_y1 = e.src.y1;
        o.offset = e.buf_off; o.count = e.count;
    }
    return OCN_OK;
}

int ocn_halo_schedule(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask, const int32_t *field_ids,
                      int32_t nfields, ocn_halo_msg *out, int32_t cap, int32_t *count)
{
    return ocn_halo_schedule_deep(basin, dec, mask, field_ids, nfields, 1, out, cap, count);
}

}  // extern "C"
