// gx_api_batch.cpp -- batches of independent pairs (BASELINE configs 4 / 5):
// the one-pass batch, the four multi-pass pipelines behind batch_core_steps
// (DESIGN.md 18.6), gx_align_batch and the multi-context gx_align_batch_multi.
#include "gx_api_call.h"

using Procs = std::vector<std::pair<const uint8_t*, const uint8_t*>>;

// Staging shared by every driver below.

// The pairs of one set that have an interior: what a fill launch is given.
struct DevPairs {
    std::vector<PairHost> ph;
    Procs proc;
    std::vector<size_t> o1, o2;   // their offsets into the staged chars (empty: every fill uploads its chars)
};
static std::vector<size_t> interior(const std::vector<PairHost>& ph) {   // pairs with an interior go to the device
    std::vector<size_t> idx;
    for (size_t p = 0; p < ph.size(); ++p) if (ph[p].n >= 1 && ph[p].m >= 1) idx.push_back(p);
    return idx;
}
static DevPairs dev_pairs(const PassSet& s, bool staged, const std::vector<size_t>& idx) {
    DevPairs d;
    for (size_t p : idx) {
        d.ph.push_back((*s.ph)[p]);
        d.proc.push_back((*s.proc)[p]);
        if (staged) { d.o1.push_back((*s.off1)[p]); d.o2.push_back((*s.off2)[p]); }
    }
    return d;
}
static SmallAlpha alpha_of(const DevPairs& d, const SmallAlpha* staged) {
    SmallAlpha alpha;
    if (staged) return *staged;
    for (size_t k = 0; k < d.proc.size() && alpha.n <= 4; ++k) {
        alpha.add(d.proc[k].first, d.ph[k].n);
        alpha.add(d.proc[k].second, d.ph[k].m);
    }
    return alpha;
}
static std::vector<int> dev_index(size_t P, const std::vector<size_t>& idx) {   // pair -> its place among the device pairs
    std::vector<int> dev_of(P, -1);
    for (size_t k = 0; k < idx.size(); ++k) dev_of[idx[k]] = (int)k;
    return dev_of;
}

// The pair sets by pass parity (one set unless alt: pass k runs set k & 1).
struct PassSets {
    PassSet v[2];
    PassSets(const PassSet& first, const PassSet* alt) : v{first, alt ? *alt : first} {}
    const PassSet& operator[](int k) const { return v[k & 1]; }
};

// What every fill of one call shares, and the fill of a DevPairs into a job.
struct FillArgs {
    gx_context* ctx;
    const Scores32& sc;
    int is_local;
    bool planes, track;
    const uint8_t* chars_dev;   // the staged chars (nullptr: see DevPairs)
    SmallAlpha alpha;
};
static int fill_dev(const FillArgs& a, const DevPairs& d, FillJob& job, int slot = -1, bool collect = true) {
    return run_fill(a.ctx, d.proc, d.ph, a.sc, a.is_local, a.planes, a.track, false, job, a.chars_dev,
                    a.chars_dev ? &d.o1 : nullptr, a.chars_dev ? &d.o2 : nullptr, &a.alpha, slot, collect);
}

// One pass's results on the host, by pair: the fills' and the start cells found from them.
struct Cells {
    std::vector<PairRes> res;
    std::vector<uint64_t> si, sj;
    std::vector<int64_t> score;
    explicit Cells(size_t P) : res(P, PairRes{}), si(P), sj(P), score(P) {}
    void take(const FillJob& j, const std::vector<size_t>& idx) {   // a fill of the device pairs idx
        for (size_t k = 0; k < idx.size(); ++k) res[idx[k]] = j.res[k];
    }
    // start cells of all pairs (sin: from these, the int64 fill's, and not from res)
    void start(const HostScores& hs, int is_local, const std::vector<PairHost>& ph, const std::vector<StartIn>* sin = nullptr) {
        for (size_t p = 0; p < ph.size(); ++p)
            start_cell_common(hs, is_local, ph[p].n, ph[p].m, sin ? (*sin)[p] : start_in(res[p]), &si[p], &sj[p], &score[p]);
    }
};
// TbStarts of the device pairs idx: from the start cells, or, without cells, a
// global batch's (n, m) with its landing column read on the device.
static void tb_starts(const std::vector<size_t>& idx, const std::vector<PairHost>& ph, int is_local, const Cells* c,
                      std::vector<TbStart>& starts) {
    starts.resize(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) {
        const size_t p = idx[k];
        if (!c) starts[k] = TbStart{(int)ph[p].n, (int)ph[p].m, 0};
        else
            starts[k] = (c->si[p] >= 1 && c->sj[p] >= 1)
                            ? TbStart{(int)c->si[p], (int)c->sj[p], is_local ? c->res[p].lmax_E : c->res[p].end_E}
                            : TbStart{0, 0, 0};
    }
}
// A GX_STAGED_KEEP_PLANES run's last fill, held back from the pool: kept once its stream is idle.
static void keep_if_held(gx_context* ctx, FillJob& j, bool held, const std::vector<int>& dev_of) {
    if (!held) return;
    (void)hipStreamSynchronize(ctx->stream);
    keep_job(ctx, j, dev_of);
}

// An overlapped pipeline that cannot run the batch (nothing left enqueued): the caller then runs the plain pipeline.
static constexpr int kOverlapNo = -1000;

// The FillJobs of one pipeline and its exits, as DevCall is for a device call
// (gx_api_call.h): every return goes through done(rc), GX_TRY included, and
// the destructor is a failing exit.  A failing exit waits for every stream a
// pipeline can have put work on before a buffer returns to the pool; a
// successful one does what its pipeline says and nothing more.
struct BatchScope {
    gx_context* const ctx;
    FillJob jobs[3];                    // the pipeline's fills in flight
    FillJob plan[2];                    // plan-only fills (no buffers): the overlapped schemes' admission check
    const size_t off0;                  // the caller's pass offset, back on every exit
    unsigned long long* const sums0;    // where the call's first checksums go
    bool open = true;

    explicit BatchScope(gx_context* c) : ctx(c), off0(c->pass_off), sums0(c->sums_dst) {}
    BatchScope(const BatchScope&) = delete;
    BatchScope& operator=(const BatchScope&) = delete;
    ~BatchScope() { done(GX_EHIP); }
    // The fill and walk streams idle, every job and every slot's held buffers
    // back in the pool (release_slots waits for the copy stream).  A job
    // handed to keep_job was swapped for an empty one.
    void drain() {
        for (hipStream_t s : {ctx->stream, ctx->stream2, ctx->tstream}) (void)hipStreamSynchronize(s);
        for (FillJob& j : jobs) job_release(ctx, j);
        release_slots(ctx);
    }
    int done(int rc) {
        if (!open) return rc;
        open = false;
        if (rc != GX_OK) {
            (void)hipStreamSynchronize(ctx->pstream);   // (a post_aside pass's reductions read its job's buffers)
            drain();
            if (rc == kOverlapNo) ctx->sums_dst = sums0;   // (the plain pipeline writes this pass's checksums again)
            ctx->post_aside = false;
        }
        ctx->pass_off = off0;
        return rc;
    }
    int refuse() {   // kOverlapNo before anything was enqueued: nothing to wait for
        open = false;
        ctx->pass_off = off0;
        return kOverlapNo;
    }
};

// The one-pass batch: fill, host start cells, device traceback, host labelling.
// Synchronous, on the context's stream.  sc == nullptr: through the int64 fill
// (jobs outside the exact-int32 range).  The staged benchmark path hands in the
// device chars and their alphabet.
static int batch_core(gx_context* ctx, const std::vector<PairHost>& ph, const Procs& proc, const HostScores& hs,
                      const Scores32* sc, int is_local, bool planes, bool track, std::vector<Walk>& walks,
                      double* fill_ms, const uint8_t* chars_dev = nullptr, const std::vector<size_t>* off1 = nullptr,
                      const std::vector<size_t>* off2 = nullptr, const SmallAlpha* staged_alpha = nullptr) {
    const size_t P = ph.size();
    const std::vector<size_t> idx = interior(ph);
    const DevPairs d = dev_pairs(PassSet{&ph, &proc, off1, off2, &walks, ctx->pass_off}, chars_dev != nullptr, idx);
    BatchScope sp(ctx);
    FillJob& job = sp.jobs[0];
    std::vector<StartIn> sin(P, StartIn{0, 0, 0, 0});
    TbOut& tb = ctx->tb_cache;
    if (!sc) tb.ms = 0;   // (the int32 path reports the cached walk's time for a batch without an interior)
    std::vector<TbStart> starts;
    Cells c(P);
    int rc = GX_OK;
    using clk = std::chrono::steady_clock;
    const auto c0 = clk::now();
    if (!idx.empty()) {
        rc = sc ? fill_dev(FillArgs{ctx, *sc, is_local, planes, track, chars_dev, alpha_of(d, staged_alpha)}, d, job)
                : run_fill_wide(ctx, d.proc, d.ph, hs, is_local, planes, track, false, job);
        if (rc) return sp.done(rc);
        c.take(job, idx);
        for (size_t k = 0; k < idx.size(); ++k) sin[idx[k]] = start_in(job, k);
    }
    const auto c1 = clk::now();
    c.start(hs, is_local, ph, &sin);
    if (!idx.empty()) {
        tb_starts(idx, ph, is_local, &c, starts);
        rc = run_traceback(ctx, job, starts, tb);
    }
    const auto c2 = clk::now();
    if (fill_ms) *fill_ms = job.fill_ms;
    if (rc) return sp.done(rc);
    const std::vector<int> dev_of = dev_index(P, idx);
    const double fms = job.fill_ms, tbms = tb.ms;
    bool held = false;
    release_or_hold(ctx, job, true, &held);
    keep_if_held(ctx, job, held, dev_of);
    // (a kept job was swapped for an empty one: the labels of a GX_STAGED_KEEP_PLANES pass carry no fill time)
    rc = label_batch(ctx, ph, hs, is_local, track, dev_of, c.si, c.sj, c.score, c.res, tb, held ? 0.0 : fms, walks);
    if (const char* e = getenv("GX_LOG"); sc && e && !strcmp(e, "debug")) {   // host-side phase times of the batch path
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[gx DEBUG] batch P=%zu fill %.3f ms (kernel %.3f) traceback %.3f ms (kernel %.3f) "
                        "label %.3f ms\n", P, ms(c0, c1), held ? 0.0 : fms, ms(c1, c2), tbms, ms(c2, clk::now()));
    }
    return sp.done(rc);
}
int batch_core_wide(gx_context* ctx, const std::vector<PairHost>& ph, const Procs& proc, const HostScores& hs,
                    int is_local, bool planes, bool track, std::vector<Walk>& walks, double* fill_ms) {
    return batch_core(ctx, ph, proc, hs, nullptr, is_local, planes, track, walks, fill_ms);
}

// One batch_core_steps call (`nsteps` passes over the same batch, the staged benchmark path) as its
// pipelines see it.  Walks and results are those of the last pass; *fill_ms is the mean fill time.
struct BatchCall {
    FillArgs fa;
    const HostScores& hs;
    int nsteps;
    PassSets sets;
    std::vector<size_t> idx;   // set 0's pairs with an interior (both sets hold the same shapes)
    double* fill_ms;
};
// Pass k's labelling, into its set's walks and rows of the pass results.
static int label_pass(const BatchCall& b, int k, const std::vector<int>& dev_of, const Cells& c, const TbOut& tb, double fill_ms,
                      const std::vector<const TbOut*>* tb_of = nullptr) {
    const PassSet& v = b.sets[k];
    b.fa.ctx->pass_off = v.pass_off;
    return label_batch(b.fa.ctx, *v.ph, b.hs, b.fa.is_local, b.fa.track, dev_of, c.si, c.sj, c.score, c.res, tb, fill_ms, *v.walks, tb_of);
}

// Unpipelined: one one-pass batch a pass.
static int steps_one_pass(const BatchCall& b, const SmallAlpha* staged_alpha) {
    gx_context* const ctx = b.fa.ctx;
    BatchScope sp(ctx);
    const int passes = std::max(b.nsteps, 1);
    double f = 0, fsum = 0;
    for (int s = 0; s < passes; ++s) {
        const PassSet& v = b.sets[s];
        ctx->pass_off = v.pass_off;
        const int rc = batch_core(ctx, *v.ph, *v.proc, b.hs, &b.fa.sc, b.fa.is_local, b.fa.planes, b.fa.track, *v.walks, &f,
                                  b.fa.chars_dev, v.off1, v.off2, staged_alpha);
        if (rc) return sp.done(rc);
        fsum += f;
    }
    if (b.fill_ms) *b.fill_ms = fsum / passes;
    return sp.done(GX_OK);
}

// Local batches, pipelined one batch deep: batch k+1's fill is queued behind
// batch k's traceback, so the host labels batch k while the device fills batch
// k+1.  Device buffers go back to the pool as soon as their last user is queued
// (everything runs on one stream); pinned staging and events alternate between
// two slots.
static int pipeline_two_slot(const BatchCall& b, const DevPairs (&d)[2]) {
    gx_context* const ctx = b.fa.ctx;
    const std::vector<PairHost>& ph = *b.sets[0].ph;
    const std::vector<size_t>& idx = b.idx;
    const size_t P = ph.size();
    const int nsteps = b.nsteps, is_local = b.fa.is_local;
    BatchScope sp(ctx);
    FillJob* const jobs = sp.jobs;
    std::vector<TbStart> starts;
    Cells c(P);
    const std::vector<int> dev_of = dev_index(P, idx);
    double fsum = 0;
    auto fill = [&](int s) { return fill_dev(b.fa, d[s], jobs[s], s, false); };   // slot s = the pass's parity = its pair set
    // results of slot s's fill -> start cells -> its traceback queued; the fill
    // buffers return to the pool (their last user, the traceback, is queued)
    int pl_pass = 0;
    bool held[2] = {false, false};
    auto trace = [&](int s) {
        int r = fill_collect(ctx, jobs[s]);
        if (r) return r;
        fsum += jobs[s].fill_ms;
        c.take(jobs[s], idx);
        c.start(b.hs, is_local, ph);
        tb_starts(idx, ph, is_local, &c, starts);
        r = run_traceback(ctx, jobs[s], starts, ctx->slots[s].out, s, false);
        release_or_hold(ctx, jobs[s], pl_pass++ == nsteps - 1, &held[s]);
        return r;
    };
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    double t_fill = 0, t_tbwait = 0, t_label = 0, t_trace = 0;   // host time per phase (GX_LOG=debug)
    const auto t_all = clk::now();
    int rc = fill(0);
    if (!rc) rc = trace(0);
    for (int k = 0; k < nsteps && !rc; ++k) {
        const int s = k & 1;
        auto t = clk::now();
        if (k + 1 < nsteps && (rc = fill(s ^ 1))) break;       // queued behind batch k's traceback
        t_fill += since(t); t = clk::now();
        if ((rc = tb_collect(ctx, s, idx.size(), ctx->slots[s].out))) break;
        t_tbwait += since(t); t = clk::now();
        if ((rc = label_pass(b, s, dev_of, c, ctx->slots[s].out, jobs[s].fill_ms))) break;
        t_label += since(t); t = clk::now();
        if (k + 1 < nsteps && (rc = trace(s ^ 1))) break;
        t_trace += since(t);
    }
    if (const char* e = getenv("GX_LOG"); e && !strcmp(e, "debug"))
        fprintf(stderr, "[gx DEBUG] pipelined %d steps P=%zu: %.3f ms/step; host per step: fill enqueue %.3f, "
                        "traceback wait %.3f, label %.3f, fill wait + traceback enqueue %.3f ms\n",
                nsteps, P, since(t_all) / nsteps, t_fill / nsteps, t_tbwait / nsteps, t_label / nsteps,
                t_trace / nsteps);
    if (rc) return sp.done(rc);
    for (int s = 0; s < 2; ++s) keep_if_held(ctx, jobs[s], held[s], dev_of);
    if (b.fill_ms) *b.fill_ms = fsum / nsteps;
    return sp.done(GX_OK);
}

// Global batches: every start cell is (n, m) and its landing column is read
// on the device, so each step's traceback is queued right behind its fill; the
// fill results (with a tracked fill's max cell and matches_at_max, which do
// not move the start) are collected on the host only for the labelling (no
// host round trip between fill and traceback; tracked Covid 5.10 -> 4.89 ms a
// step at a 4.74 ms fill).
//
// Three slots in flight: pass k+2's fill and walk are queued before the host
// waits for pass k's records, so the record copy (4.3 MB on a 1024 x 1k pass,
// ~0.22 ms on the copy engine after the walk) and the labelling (~0.52 ms) of
// pass k run beside passes k+1 and k+2 on the device.  One slot ahead, the
// next fill was queued only after the labelling: the device sat idle ~0.2 ms a
// pass (rocprofv3 timeline, 1024 x 1k).  A slot's pinned buffers are rewritten
// when pass k+3 is queued, after pass k was labelled; its device descriptor
// caches on the fill stream, in stream order.
static int pipeline_three_slot(const BatchCall& b, const DevPairs (&d)[2]) {
    gx_context* const ctx = b.fa.ctx;
    const std::vector<PairHost>& ph = *b.sets[0].ph;
    const std::vector<size_t>& idx = b.idx;
    const size_t P = ph.size();
    const int nsteps = b.nsteps, is_local = b.fa.is_local;
    BatchScope sp(ctx);
    FillJob* const jobs = sp.jobs;
    std::vector<TbStart> starts;   // (n, m): the same every pass
    tb_starts(idx, ph, is_local, nullptr, starts);
    Cells c(P);
    const std::vector<int> dev_of = dev_index(P, idx);
    double fsum = 0;
    // the walk stays on the fill's stream: the fill's buffers return to
    // the pool right behind it (stream-ordered reuse).  (A walk on its own
    // stream beside the next step's fill, its buffers released once the
    // walk is collected, measured in round 5 (tools/walk_stream_sweep.sh,
    // 3 alternating runs a size): 1024 x 1k 0.99 -> 1.06 ms a step,
    // 1024 x 4k 8.35 -> 8.17, 128 x 16k 17.5 -> 17.6: the walk and the
    // fill slow each other down on shared CUs (fill 0.56 -> 0.67 ms beside
    // a walk stretched from 0.30 to 0.82), and the host's labelling then
    // leaves the device idle between pairs of steps.)
    int tr_pass = 0;
    bool held[3] = {false, false, false};
    // the walk on its own stream beside the next pass's fill, when the
    // two more passes' fill buffers this holds (a walk keeps its fill's
    // buffers until it is collected) fit the free HBM as it is -- not by
    // evicting the pool's cached buffers, whose re-allocation costs far
    // more (hipMalloc of an 86 GB plane buffer ~2.4 s: a 4-pair 64k batch
    // that evicted them cost the next 1024 x 64k batch 7 s).  1024 x 1k
    // 0.94 -> 0.84 ms a pass, 1024 x 4k 7.93 -> 7.57 (tools/walk_prio_ab.sh).
    // (With one slot ahead it was slower: the labelling, not the device,
    // then set the pace.)  GX_TB_OWN_STREAM=0 keeps the walk on the fill's
    // stream.
    bool wstream = !ctx->keep_capture && !(getenv("GX_TB_OWN_STREAM") && !strcmp(getenv("GX_TB_OWN_STREAM"), "0"));
    if (wstream) {
        double need = 0;
        for (const PairHost& h : d[0].ph) need += pair_device_bytes(h.n, h.m, 2.0);
        size_t fr = 0, tot = 0;
        wstream = hipMemGetInfo(&fr, &tot) == hipSuccess && 2.0 * need <= (double)fr - 4.0 * (1ull << 30);
    }
    bool jheld[3] = {false, false, false};
    auto trace_dev = [&](int s) {
        if (wstream) {   // the walk on its own stream; the fill's buffers held until it is collected
#ifndef GX_MUT_NO_FDONE_WAIT   // (mutation build only: tests/test_gpu_atsize.py must catch its absence)
            // (on the fill kernel's own end event: the walk needs its planes
            // and end cell only, not the reductions queued after it -- a
            // tracked fill's max column and matches_at_max -- nor the
            // checksums of a staged parity pass)
            if (hipStreamWaitEvent(ctx->tstream, ctx->slots[s].fe, 0) != hipSuccess) return fail(GX_EHIP, "walk stream wait");
#endif
            jheld[s] = true;
            const int r = run_traceback(ctx, std::vector<const FillJob*>{&jobs[s]}, starts, ctx->slots[s].out, s, false,
                                        true, ctx->tstream);
#ifdef GX_MUT_EARLY_RELEASE   // (mutation build only: the fill's buffers back to the pool while the walk may read them)
            job_release(ctx, jobs[s]);
            jheld[s] = false;
#endif
            return r;
        }
        int r = run_traceback(ctx, jobs[s], starts, ctx->slots[s].out, s, false, true);
        release_or_hold(ctx, jobs[s], tr_pass++ == nsteps - 1, &held[s]);   // stream order: later users come after the traceback
        return r;
    };
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    const auto t_all = clk::now();
    double h_enq = 0, h_tbw = 0, h_res = 0, h_lab = 0;   // host time per phase (GX_LOG=debug)
    int queued = 0;   // passes whose fill and walk are queued
    int rc = GX_OK;
    for (int k = 0; k < nsteps && !rc; ++k) {
        const int s = k % 3;
        auto t = clk::now();
        while (!rc && queued < std::min(nsteps, k + 3)) {
            const int q = queued++;
            // (a pass's reductions beside the next fill only once the walk's
            // stream is settled: it holds the pass's buffers until collected)
            ctx->post_aside = wstream && q > 0;
            rc = fill_dev(b.fa, d[q & 1], jobs[q % 3], q % 3, false);   // slot q % 3 (pinned staging, events, job), pair set q & 1
            ctx->post_aside = false;
            if (rc) break;
            // two fill workgroups a CU (7-wave bands, run_fill) leave the
            // walks no room beside the fill: the walk stays on its stream
            if (q == 0 && ctx->last_W == 7) wstream = false;
            rc = trace_dev(q % 3);
        }
        if (rc) break;
        h_enq += since(t); t = clk::now();
        if ((rc = tb_collect(ctx, s, idx.size(), ctx->slots[s].out))) break;
        h_tbw += since(t); t = clk::now();
        if ((rc = fill_collect(ctx, jobs[s]))) break;
        fsum += jobs[s].fill_ms;
        c.take(jobs[s], idx);
        c.start(b.hs, is_local, ph);
        if (jheld[s]) { job_release(ctx, jobs[s]); jheld[s] = false; }   // its walk has ended
        h_res += since(t); t = clk::now();
        if ((rc = label_pass(b, k, dev_of, c, ctx->slots[s].out, jobs[s].fill_ms))) break;
        h_lab += since(t);
    }
    if (const char* e = getenv("GX_LOG"); e && !strcmp(e, "debug"))
        fprintf(stderr, "[gx DEBUG] pipelined %d steps P=%zu (device traceback starts): %.3f ms/step; host per step: "
                "enqueue fill+traceback %.3f, traceback wait %.3f, fill results %.3f, labelling %.3f ms\n", nsteps, P,
                since(t_all) / nsteps, h_enq / nsteps, h_tbw / nsteps, h_res / nsteps, h_lab / nsteps);
    if (rc) return sp.done(rc);
    for (int s = 0; s < 3; ++s) keep_if_held(ctx, jobs[s], held[s], dev_of);
    if (b.fill_ms) *b.fill_ms = fsum / nsteps;
    return sp.done(GX_OK);
}

// The overlapped pipelines, for an untracked batch on the twin fill without
// landing columns (the sequential strip walk, tb_seq_kernel, ~5 ms for a 30k
// pair, uses a few CUs): the pairs are split into group A (half of them; local
// batches a fifth) and group B, each filled by its own launch on its own stream.
struct Groups {
    size_t G;                    // group A's pairs
    std::vector<size_t> gi[2];   // the groups' pairs
    DevPairs d[2][2];            // [pair set][group]
};
static Groups overlap_groups(const BatchCall& b) {
    const size_t Q = b.idx.size();
    Groups g;
    // group A: half the pairs (global), even (twins).  Two equal launches
    // fill the chip better than a small A beside a large B: 80 x 30k, fill ms
    // a pass by A's pairs 8 / 16 / 24 / 32 / 40 = 33.7 / 29.9 / 29.0 / 27.0 /
    // 26.5 (the one-launch pass 27.8); all-vs-all with planes 20.4 -> 17.0 ms,
    // 1024 x 16k 100.4 -> 99.4.  Local batches keep a fifth (64 related local
    // pairs 26.9 ms against 27.9 at half; profiles/r05_overlap_split.txt).
    // GX_OVERLAP_A sets A's pair count.
    // (half rounded up: a chunked batch's 19- and 20-pair chunks then both
    // split 10 + 9 / 10 + 10 and reuse the same cached plane buffers)
    g.G = std::max<size_t>(2, (b.fa.is_local ? Q / 5 : (Q + 1) / 2) & ~(size_t)1);
    if (const char* e = getenv("GX_OVERLAP_A"); e && atoi(e) >= 2 && (size_t)atoi(e) + 2 <= Q)
        g.G = (size_t)atoi(e) & ~(size_t)1;
    g.gi[0].assign(b.idx.begin(), b.idx.begin() + (long)g.G);
    g.gi[1].assign(b.idx.begin() + (long)g.G, b.idx.end());
    for (int v = 0; v < 2; ++v)
        for (int k = 0; k < 2; ++k) g.d[v][k] = dev_pairs(b.sets[v], b.fa.chars_dev != nullptr, g.gi[k]);
    return g;
}
// Both groups must take the twin fill without landing columns, in one format:
// decided from plan-only fills, before anything is enqueued.
static bool overlap_admits(const BatchCall& b, const Groups& g, BatchScope& sp) {
    FillJob &pa = sp.plan[0], &pb = sp.plan[1];
    pa.plan_only = pb.plan_only = true;
    int prc = fill_dev(b.fa, g.d[0][0], pa, 0, false);
    if (!prc) prc = fill_dev(b.fa, g.d[0][1], pb, 2, false);
    return !prc && pa.noskel && pb.noskel && pa.twin && pb.twin && pa.lay == pb.lay && pa.rows == pb.rows;
}

// Scheme 2, the rotation: global batches on the half split rotate three plane
// buffers (overlap_rotate_plan).  The fills are numbered i = 2 pass + group and
// alternate between the two fill streams; fill i runs in FillJob i % 3, and
// its pairs alone are walked on tstream behind it (the walk waits for that
// fill's fdone only, so group A's walk of a pass does not wait for group B's
// fill).  Before fill i is enqueued the host has collected fill i - 3's
// results and put its buffers back into the pool, and fill i's stream waits on
// the device for the end of walk i - 3, the last reader of those buffers (the
// walks share one stream, so that wait covers every earlier walk: any stream
// may take what the pool holds once it has waited so).  Every device-side
// wait names work enqueued earlier, with a smaller fill index: fill i waits
// for walk i - 3, walk i for fill i, and both for their stream predecessors,
// so the waits cannot form a cycle; inside a launch the band queue's order
// guarantees progress, and launches do not depend on each other otherwise.
// In steady state walk i - 3 ended two launches before fill i can start, so
// no fill waits for a walk (the two-buffer scheme's B fill stood ~5 ms a pass
// behind the whole pass's walk).  Three consecutive groups are alive at once
// (A, B, A or B, A, B), every job holding a buffer of the larger group's
// size: 3 x (Q / 2 + 2) pairs of a Q-pair batch at most, 1.5 P on the
// headline, 3 x 10 = 1.67 P at Q = 18 (A = 8, B = 10): at 1.5 B a cell of twin
// codes <= 2.25 + 9 / Q <= 2.82 B a cell of the batch from Q = 16, within the
// 3.25 B a cell the chunk plan budgets for a pair of a compact-plane batch.
// The host labels pass k once both its walks are collected, after it has
// enqueued fill 2k + 4; walk records stay in their slot until then (slot
// i % 6).  GX_OVERLAP_ROTATE=0 keeps global batches on scheme 1.
RotatePlan overlap_rotate_plan(int i) {
    RotatePlan r;
    r.job = i % 3;
    r.fslot = 2 * (i & 1) + ((i >> 1) & 1);   // (a stream's two slots: run_fill looks a descriptor block up in slot and slot ^ 1)
    r.wslot = i % 6;
    r.stream = i & 1;
    r.wait_walk = i >= 3 ? i - 3 : -1;
    r.collected = i >= 3 ? i - 3 : -1;
    // pass k is labelled after fill 2k + 4 was enqueued: before fill i, the passes up to (i - 5) / 2
    r.labelled = i >= 5 ? 2 * ((i - 5) / 2) + 1 : -1;
    return r;
}
extern "C" int gx_overlap_rotate_plan(int fill, int* out7) {
    if (fill < 0 || !out7) return fail(GX_EINVAL, "gx_overlap_rotate_plan: fill < 0 or out is NULL");
    const RotatePlan r = overlap_rotate_plan(fill);
    const int v[7] = {r.job, r.fslot, r.wslot, r.stream, r.wait_walk, r.collected, r.labelled};
    std::copy(v, v + 7, out7);
    return GX_OK;
}
extern "C" int gx_overlap_scheme(const gx_context* ctx) { return ctx ? ctx->last_scheme : -1; }

static int pipeline_rotate(const BatchCall& b, const Groups& g, BatchScope& sp) {
    gx_context* const ctx = b.fa.ctx;
    const std::vector<PairHost>& ph = *b.sets[0].ph;
    const size_t P = ph.size();
    hipStream_t const sT = ctx->tstream;
    const FillJob& pa = sp.plan[0];
    FillJob* const jobs = sp.jobs;   // three jobs, each with room for the larger group
    for (int k = 0; k < 3; ++k) jobs[k].plane_floor = std::max(pa.plane_bytes, sp.plan[1].plane_bytes);
    const int N = 2 * b.nsteps;
    Cells c(P);
    std::vector<TbStart> gstarts[2];
    std::vector<int> gdev(P, -1);   // a pair's index in its group's walk
    for (int k = 0; k < 2; ++k) {
        tb_starts(g.gi[k], ph, 0, nullptr, gstarts[k]);
        for (size_t q = 0; q < g.gi[k].size(); ++q) gdev[g.gi[k][q]] = (int)q;
    }
    std::vector<const TbOut*> tb_of(P, nullptr);
    double fms[6] = {0, 0, 0, 0, 0, 0};   // fill i's kernel time, by its walk slot
    auto enqueue = [&](int i) -> int {   // fill i and, behind it, the walk of its pairs
        const RotatePlan rp = overlap_rotate_plan(i);
        FillJob& j = jobs[rp.job];
        hipStream_t const fs = rp.stream ? ctx->stream2 : ctx->stream;
        if (i == 0) GX_TRY(sp, hipEventRecord(ctx->ev0, fs));
#ifndef GX_MUT_NO_ROTATE_WAIT   // (mutation build only: the refill no longer ordered behind the job's last walk)
        if (rp.wait_walk >= 0) GX_TRY(sp, hipStreamWaitEvent(fs, ctx->slots[overlap_rotate_plan(rp.wait_walk).wslot].te, 0));
#endif
        j.stream = fs;
        const int r = fill_dev(b.fa, g.d[(i >> 1) & 1][i & 1], j, rp.fslot, false);
        if (r) return r;
        // (only if the plan-only fill and the real fill of the same inputs disagree; kOverlapNo drains through done())
        if (!(j.noskel && j.twin && j.lay == pa.lay && j.rows == pa.rows))
            return i < 2 ? kOverlapNo : fail(GX_EHIP, "overlapped batch: fill formats changed");
        if (i == N - 1) {   // the last fill's end, behind the one before it on the other stream
            GX_TRY(sp, hipStreamWaitEvent(fs, ctx->slots[overlap_rotate_plan(i - 1).fslot].fdone, 0));
            GX_TRY(sp, hipEventRecord(ctx->ev1, fs));
        }
        GX_TRY(sp, hipStreamWaitEvent(sT, ctx->slots[rp.fslot].fdone, 0));
        // (walk i runs beside fills i + 1 and i + 2; the call's last walk beside nothing: walk_policy)
        return run_traceback(ctx, std::vector<const FillJob*>{&j}, gstarts[i & 1], ctx->slots[rp.wslot].out, rp.wslot,
                             false, false, sT, i + 1 < N);
    };
    // fill i's results; its buffers back to the pool, though walk i may
    // still read them: their next user's stream waits for that walk
    auto collect = [&](int i) -> int {
        const RotatePlan rp = overlap_rotate_plan(i);
        FillJob& j = jobs[rp.job];
        const int r = fill_collect(ctx, j);
        if (r) return r;
        fms[rp.wslot] = j.fill_ms;
        c.take(j, g.gi[i & 1]);
        job_release(ctx, j);
        return GX_OK;
    };
    auto label = [&](int k) -> int {   // pass k: both groups' records, then the labelling
        for (int q = 0; q < 2; ++q) {
            const int ws = overlap_rotate_plan(2 * k + q).wslot;
            const int r = tb_collect(ctx, ws, g.gi[q].size(), ctx->slots[ws].out);
            if (r) return r;
            for (size_t p : g.gi[q]) tb_of[p] = &ctx->slots[ws].out;
        }
        c.start(b.hs, 0, ph);
        const int w0 = overlap_rotate_plan(2 * k).wslot, w1 = overlap_rotate_plan(2 * k + 1).wslot;
        return label_pass(b, k, gdev, c, ctx->slots[w0].out, fms[w0] + fms[w1], &tb_of);
    };
    int rc = GX_OK;
    for (int t = 0; t < N + 3 && !rc; ++t) {
        if (t >= 3) rc = collect(t - 3);
        if (!rc && t < N) rc = enqueue(t);
        if (!rc && t >= 3 && ((t - 3) & 1)) rc = label((t - 3) / 2);
    }
    if (rc) return sp.done(rc);
    // the fills' time per step: the whole fill pipeline (the first fill's start to the last fill's end, ev0..ev1) over the steps
    GX_TRY(sp, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    GX_TRY(sp, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    sp.drain();
    ctx->last_groups = 2;
    ctx->last_scheme = 2;
    if (b.fill_ms) *b.fill_ms = (double)ms / b.nsteps;
    return sp.done(GX_OK);
}

// Scheme 1: local batches (a fifth against four fifths: rotation would hold
// 1.8 P) and batches split by GX_OVERLAP_A keep two A buffers and one B buffer:
// step k's walk (stream tstream, after both fills) runs beside step k+1's
// group-A fill, whose plane codes go to a second A buffer (the device holds
// P + |A| pairs' planes); step k+1's group-B fill waits on the device for step
// k's walk before it reuses B's buffers.  Only buffers no pending work uses go
// back to the pool (a walk's fills after it was collected; B's before its next
// fill, which waits for the walk that reads them), so any stream may take them.
static int pipeline_two_buffer(const BatchCall& b, const Groups& g, BatchScope& sp) {
    gx_context* const ctx = b.fa.ctx;
    const std::vector<PairHost>& ph = *b.sets[0].ph;
    const size_t P = ph.size(), Q = b.idx.size();
    const int nsteps = b.nsteps, is_local = b.fa.is_local;
    hipStream_t const sA = ctx->stream, sB = ctx->stream2, sT = ctx->tstream;
    FillJob* const jA = sp.jobs;   // group A's two buffers, by step parity
    FillJob& jB = sp.jobs[2];
    const std::vector<int> dev_of = dev_index(P, b.idx);   // (b.idx is group A's pairs, then group B's)
    std::vector<TbStart> starts;
    tb_starts(b.idx, ph, is_local, nullptr, starts);
    Cells c(P);
    auto fill = [&](int k, int step) {   // group k's fill of a step
        FillJob& j = k == 0 ? jA[step & 1] : jB;
        j.stream = k == 0 ? sA : sB;
        return fill_dev(b.fa, g.d[step & 1][k], j, 2 * k + (step & 1), false);
    };
    auto trace = [&](int step) -> int {
        GX_TRY(sp, hipStreamWaitEvent(sT, ctx->slots[step & 1].fdone, 0));
        GX_TRY(sp, hipStreamWaitEvent(sT, ctx->slots[2 + (step & 1)].fdone, 0));
        // (local: the start cells are read on the device, TbDev.start_ij_dev)
        return run_traceback(ctx, std::vector<const FillJob*>{&jA[step & 1], &jB}, starts, ctx->slots[step & 1].out, step & 1,
                             false, is_local != 0, sT);
    };
    GX_TRY(sp, hipEventRecord(ctx->ev0, sA));
    int rc = fill(0, 0);
    if (!rc) rc = fill(1, 0);
    // (only if the plan-only fills and the real fills of the same inputs disagree; done() drains them)
    if (!rc && !(jA[0].noskel && jB.noskel && jA[0].lay == jB.lay && jA[0].twin && jB.twin && jA[0].rows == jB.rows))
        return sp.done(kOverlapNo);
    if (!rc) rc = trace(0);
    // the fills' time per step: one step's fills overlap the next step's and
    // the walks, so the whole fill pipeline (the first fill's start to the
    // last fill's end, ev0..ev1) over the steps
    float fspan = 0.f;
    for (int k = 0; k < nsteps && !rc; ++k) {
        const int a = k & 1;
        if (k + 1 < nsteps) {
            if ((rc = fill(0, k + 1))) break;                 // beside step k's walk (its buffers: step k-1's, collected)
            if ((rc = fill_collect(ctx, jB))) break;          // step k's group B, before jB is refilled
            c.take(jB, g.gi[1]);
            job_release(ctx, jB);                             // read by step k's walk: the next B fill waits for it
            GX_TRY(sp, hipStreamWaitEvent(sB, ctx->slots[a].te, 0));
            if ((rc = fill(1, k + 1))) break;
            if (k + 2 == nsteps) {                            // behind the last fill (B's comes after A's, below)
                GX_TRY(sp, hipStreamWaitEvent(sB, ctx->slots[(k + 1) & 1].fdone, 0));
                GX_TRY(sp, hipEventRecord(ctx->ev1, sB));
            }
            if (!(jA[(k + 1) & 1].noskel && jB.noskel)) { rc = fail(GX_EHIP, "overlapped batch: fill formats changed"); break; }
            if ((rc = trace(k + 1))) break;
        } else {
            if ((rc = fill_collect(ctx, jB))) break;
            c.take(jB, g.gi[1]);
        }
        if ((rc = fill_collect(ctx, jA[a]))) break;
        c.take(jA[a], g.gi[0]);
        if (k + 1 == nsteps) {
            GX_TRY(sp, hipEventSynchronize(ctx->ev1));
            GX_TRY(sp, hipEventElapsedTime(&fspan, ctx->ev0, ctx->ev1));
        }
        if ((rc = tb_collect(ctx, a, Q, ctx->slots[a].out))) break;
        job_release(ctx, jA[a]);                              // its walk is done
        c.start(b.hs, is_local, ph);
        if ((rc = label_pass(b, a, dev_of, c, ctx->slots[a].out, jA[a].fill_ms + jB.fill_ms))) break;
    }
    if (rc) return sp.done(rc);
    sp.drain();
    ctx->last_groups = 2;
    ctx->last_scheme = 1;
    if (b.fill_ms) *b.fill_ms = (double)fspan / nsteps;
    return sp.done(GX_OK);
}

// Returns kOverlapNo (nothing left enqueued) when the two groups' fills do not
// both take the twin fill without landing columns.
static int pipeline_overlapped(const BatchCall& b) {
    const Groups g = overlap_groups(b);
    BatchScope sp(b.fa.ctx);
    if (!overlap_admits(b, g, sp)) return sp.refuse();
    const size_t Q = b.idx.size();
    const char* rot_e = getenv("GX_OVERLAP_ROTATE");
    if (!b.fa.is_local && g.G == std::max<size_t>(2, ((Q + 1) / 2) & ~(size_t)1) && !(rot_e && !strcmp(rot_e, "0")))
        return pipeline_rotate(b, g, sp);
    return pipeline_two_buffer(b, g, sp);
}

// The chooser: unpipelined, overlapped where it pays, else the plain pipeline
// of the batch's kind.
int batch_core_steps(gx_context* ctx, const std::vector<PairHost>& ph, const Procs& proc, const HostScores& hs,
                     const Scores32& sc, int is_local, bool planes, bool track, int nsteps,
                     std::vector<Walk>& walks, double* fill_ms, const uint8_t* chars_dev,
                     const std::vector<size_t>* off1, const std::vector<size_t>* off2,
                     const SmallAlpha* staged_alpha, const PassSet* alt) {
    ctx->last_groups = 1;
    ctx->last_scheme = 0;
    BatchCall b{FillArgs{ctx, sc, is_local, planes, track, chars_dev, SmallAlpha{}}, hs, nsteps,
                PassSets(PassSet{&ph, &proc, off1, off2, &walks, ctx->pass_off}, alt), interior(ph), fill_ms};
    if (nsteps <= 1 || b.idx.empty() || getenv("GX_TRACE_FILE")) return steps_one_pass(b, staged_alpha);
    const int rc = slots_ready(ctx);
    if (rc) return fail(rc, "pipeline events");
    const DevPairs d[2] = {dev_pairs(b.sets[0], chars_dev != nullptr, b.idx), dev_pairs(b.sets[1], chars_dev != nullptr, b.idx)};
    b.fa.alpha = alpha_of(d[0], staged_alpha);
    size_t nmax_b = 0;
    for (const PairHost& h : d[0].ph) nmax_b = std::max(nmax_b, h.n);
    // (long pairs only: a short pair's walk is short; and both groups must
    // fill the grid on the twin fill, or the attempt falls back.  1024 x 4k:
    // 14.9 ms a step overlapped against 10.8 plain; 1024 x 16k 116.8 against
    // 145, measured in round 4 (those records were replaced by the round-5
    // ones on the same rule, profiles/r05_config5_*.json; the plain-pipeline
    // side: profiles/r02k_config5_*.json))
    // (local batches from 64 pairs: at 32 related 30k pairs the split launches
    // fill worse than the walk they hide, 27.2 vs 21.6 ms a step; GX_OVERLAP=1
    // forces it from 16 pairs, GX_OVERLAP=0 turns it off)
    const char* ov = getenv("GX_OVERLAP");
    const bool ov_force = ov && !strcmp(ov, "1");
    if (!track && planes && b.idx.size() >= 16 && (nmax_b >= 16384 || ov_force) && !ctx->keep_capture &&
        !(ov && !strcmp(ov, "0")) && (!is_local || b.idx.size() >= 64 || ov_force)) {
        const int orc = pipeline_overlapped(b);
        if (orc != kOverlapNo) return orc;
    }
    return is_local ? pipeline_two_slot(b, d) : pipeline_three_slot(b, d);
}

extern "C" int gx_align_batch(gx_context* ctx, const uint8_t* const* s1, const size_t* n, const uint8_t* const* s2,
                              const size_t* m, size_t npairs, const gx_scores* scores, int is_local,
                              uint32_t flags, gx_step* const* steps, const size_t* caps, gx_result* out) {
    if (!ctx || !s1 || !n || !s2 || !m || !out) return fail(GX_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIPCHK(hipSetDevice(ctx->device));
    size_t nmax = 0, mmax = 0;
    for (size_t p = 0; p < npairs; ++p) { nmax = std::max(nmax, n[p]); mmax = std::max(mmax, m[p]); }
    HostScores hs;
    Scores32 sc;
    bool wide = false;
    int rc = check_scores(scores, nmax, mmax, &hs, &sc, is_local, &wide);
    if (rc) return rc;
    std::vector<PairHost> ph(npairs);
    Procs proc(npairs);
    for (size_t p = 0; p < npairs; ++p) {
        ph[p] = PairHost{s1[p], s2[p], n[p], m[p]};
        proc[p] = {s1[p], s2[p]};
    }
    // traceback codes only (no planes); batches beyond the free HBM run in
    // chunks.  Local batches that a plan of the whole batch puts on the local
    // twin fill keep its plane codes as scratch for the walk
    // (2 B/cell; chunks planned at the scalar byte format's 3 B/cell, should a
    // chunk fall back)
    bool lplanes = false;
    if (is_local && !wide && !(flags & GX_ALIGN_MAX_CELL)) {
        const DevPairs nz = dev_pairs(PassSet{&ph, &proc, nullptr, nullptr, nullptr, 0}, false, interior(ph));
        FillJob pj;
        pj.plan_only = true;
        lplanes = !nz.ph.empty() && !run_fill(ctx, nz.proc, nz.ph, sc, is_local, true, false, false, pj) && pj.twin;
    }
    const auto chunks = plan_chunks(ctx, ph, lplanes ? 3.0 : 0.0);
    ctx->last_chunks = (int)chunks.size();
    std::vector<Walk> walks;
    for (const auto& c : chunks) {
        std::vector<PairHost> phc(ph.begin() + c.first, ph.begin() + c.second);
        Procs pc(proc.begin() + c.first, proc.begin() + c.second);
        rc = batch_core(ctx, phc, pc, hs, wide ? nullptr : &sc, is_local, lplanes, (flags & GX_ALIGN_MAX_CELL) != 0, walks, nullptr);
        if (rc) return rc;
        for (size_t k = 0; k < phc.size(); ++k) {
            const size_t p = c.first + k;
            out[p] = walks[k].res;
            if (steps && steps[p]) {
                rc = copy_steps(walks[k], steps[p], caps ? caps[p] : 0);
                if (rc) return rc;
            }
        }
    }
    return GX_OK;
}

// Many independent pairs over several GPUs (one context each): the pairs are
// shared out by longest-processing-time on n * m cells (the heaviest pair to
// the least-loaded context), and each share runs as one gx_align_batch on its
// own host thread -- no device-to-device traffic, the shares are independent.
// The reference's multi-worker driver is the rayon pool over all pairs of
// compare (main.rs:245-261); this is its multi-GPU counterpart.
static std::vector<std::vector<size_t>> lpt_shares(const size_t* n, const size_t* m, size_t npairs, int parts) {
    std::vector<size_t> order(npairs);
    for (size_t p = 0; p < npairs; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return (double)n[a] * (double)m[a] > (double)n[b] * (double)m[b];
    });
    std::vector<std::vector<size_t>> bins((size_t)parts);
    std::vector<double> load((size_t)parts, 0.0);
    for (size_t p : order) {
        size_t b = 0;
        for (size_t k = 1; k < bins.size(); ++k)
            if (load[k] < load[b]) b = k;
        bins[b].push_back(p);
        load[b] += (double)n[p] * (double)m[p] + (double)(n[p] + m[p]);
    }
    for (auto& b : bins) std::sort(b.begin(), b.end());
    return bins;
}

extern "C" int gx_align_batch_multi(gx_context* const* ctxs, int nctx, const uint8_t* const* s1, const size_t* n,
                                    const uint8_t* const* s2, const size_t* m, size_t npairs,
                                    const gx_scores* scores, int is_local, uint32_t flags, gx_step* const* steps,
                                    const size_t* caps, gx_result* out) {
    if (!ctxs || nctx < 1 || !s1 || !n || !s2 || !m || !out) return fail(GX_EINVAL, "NULL argument");
    for (int k = 0; k < nctx; ++k)
        if (!ctxs[k]) return fail(GX_EINVAL, "NULL context");
    if (nctx == 1)
        return gx_align_batch(ctxs[0], s1, n, s2, m, npairs, scores, is_local, flags, steps, caps, out);
    const auto bins = lpt_shares(n, m, npairs, nctx);
    std::vector<int> rc((size_t)nctx, GX_OK);
    std::vector<std::string> err((size_t)nctx);
    std::vector<std::thread> th;
    for (int k = 0; k < nctx; ++k) {
        if (bins[(size_t)k].empty()) continue;
        th.emplace_back([&, k] {
            const auto& b = bins[(size_t)k];
            const size_t q = b.size();
            std::vector<const uint8_t*> a1(q), a2(q);
            std::vector<size_t> an(q), am(q), acap(q);
            std::vector<gx_step*> ast(q, nullptr);
            std::vector<gx_result> ares(q);
            for (size_t x = 0; x < q; ++x) {
                const size_t p = b[x];
                a1[x] = s1[p]; a2[x] = s2[p]; an[x] = n[p]; am[x] = m[p];
                ast[x] = steps ? steps[p] : nullptr;
                acap[x] = caps ? caps[p] : 0;
            }
            rc[(size_t)k] = gx_align_batch(ctxs[k], a1.data(), an.data(), a2.data(), am.data(), q, scores, is_local,
                                           flags, steps ? ast.data() : nullptr, caps ? acap.data() : nullptr,
                                           ares.data());
            if (rc[(size_t)k]) err[(size_t)k] = g_err;   // g_err is thread-local
            else
                for (size_t x = 0; x < q; ++x) out[b[x]] = ares[x];
        });
    }
    for (auto& t : th) t.join();
    for (int k = 0; k < nctx; ++k)
        if (rc[(size_t)k]) return fail(rc[(size_t)k], "context " + std::to_string(k) + ": " + err[(size_t)k]);
    return GX_OK;
}
