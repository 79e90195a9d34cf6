// gx_api_call.h -- the scope of one device call and the stages that the
// drivers of suffix-tree mode, compare mode and search mode share
// (DESIGN.md 18.5).  Host code only; no kernel includes it.
//
//   DevCall            the pooled buffers a call takes, on the context's stream;
//                      done(rc) on every exit, the destructor behind it
//   GX_TRY / GX_GET    a HIP call / a buffer, or leave through done()
//   radix_sort_pairs   the eight-pass loop over launch_suf_sort_pass
//   stage_batch        a batch's bytes, offsets, counters and pinned words
#pragma once
#include "gx_api.h"
#include "gx_suffix.h"

#pragma GCC visibility push(hidden)

// One call on ctx->stream; the caller holds ctx->mu.
struct DevCall {
    gx_context* const ctx;
    const hipStream_t st;
    std::vector<DevBuf> held;

    explicit DevCall(gx_context* c) : ctx(c), st(c->stream) { held.reserve(32); }   // (the edit search takes 25)
    DevCall(const DevCall&) = delete;
    DevCall& operator=(const DevCall&) = delete;
    ~DevCall() {   // (a forgotten done(): as a failing exit)
        if (!held.empty()) done(GX_EHIP);
    }
    // count elements of T from the context's pool, the call's until done()
    template <class T>
    int get(T*& p, size_t count) {
        DevBuf b;
        const int rc = pool_get(ctx, count * sizeof(T), &b, st);
        if (rc != GX_OK) return rc;
        held.push_back(b);
        p = (T*)b.p;
        return GX_OK;
    }
    // Every exit: a failing one first waits until nothing of this call still
    // runs on the buffers; a successful one comes with the stream idle.
    int done(int rc) {
        if (rc != GX_OK) (void)hipStreamSynchronize(st);
        for (DevBuf& b : held) pool_put(ctx, b);
        held.clear();
        return rc;
    }
    // device ms between two recorded events of a drained stream (left alone when the events cannot say)
    static void elapsed(hipEvent_t a, hipEvent_t b, double* into) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess) *into = ms;
    }
};

// `call`: a DevCall, or anything else with done(int) and get(...).  A function
// that uses them returns an int; after a non-zero return done() has run.
#define GX_TRY(call, expr)                                                                                    \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return (call).done(fail(e_ == hipErrorOutOfMemory ? GX_ENOMEM : GX_EHIP,                          \
                                    std::string(#expr) + ": " + hipGetErrorString(e_)));                      \
    } while (0)
#define GX_GET(call, ptr, count)                                                \
    do {                                                                        \
        const int rc_ = (call).get((ptr), (count));                             \
        if (rc_ != GX_OK) return (call).done(rc_);                              \
    } while (0)

// LSD radix sort of `count` (key, value) pairs over the digit bytes that
// `digits` has a bit in: pass p (bits 8p .. 8p+7) runs iff that byte of
// `digits` is non-zero, from key[*cur], val[*cur] into the other pair, which
// *cur then names.  ran (may be NULL): bit p set for every pass that ran.
// table: 256 * suf_tiles(count) words; tmp: suf_tiles of that.  (gx_api_suffix.cpp)
hipError_t radix_sort_pairs(uint64_t* const key[2], uint32_t* const val[2], uint32_t count, uint32_t* table, uint32_t* tmp,
                            uint64_t digits, hipStream_t st, int* cur, unsigned* ran = nullptr);
// The digits of keys hi << 32 | lo with lo <= lo_max and hi <= hi_max: byte p of
// a half is in while its bound >> 8p is non-zero.
inline uint64_t radix_digits(uint32_t lo_max, uint32_t hi_max) {
    uint64_t d = 0;
    for (int p = 0; p < 4; ++p) {
        if (lo_max >> (8 * p)) d |= 0xffull << (8 * p);
        if (hi_max >> (8 * p)) d |= 0xffull << (8 * (p + 4));
    }
    return d;
}

// A batch on the device as every driver of search mode stages it (gx_api_search.cpp).
struct StagedBatch {
    const uint8_t* bytes = nullptr;      // the items back to back, kSufPad zero bytes behind them
    const uint32_t* off = nullptr;       // n + 1 offsets
    unsigned long long* cnt = nullptr;   // 8 zeroed counters
    unsigned long long* pin = nullptr;   // 16 pinned words for their read-back (the context's staging block)
};
// src: total_bytes unpadded bytes; offs: n + 1 offsets.  what: the caller's name in the messages ("search").
// Both sources are pageable: the copies have left them once the stream is synchronised.
int stage_batch(DevCall& call, const char* what, const uint8_t* src, size_t total_bytes, const uint32_t* offs, uint32_t n,
                StagedBatch& b);
// The item batch of the caller's n patterns on the chosen strands (gx_strand.h): the same one
// host copy of src, the reverse items written behind it (BOTH) or beside it (REV) by the kernel of
// gx_strand.hip.  offs: the caller's n + 1 offsets (the item offsets begin with them).  FWD is stage_batch.
// Leaves gx_strand_info's numbers in the context.
int stage_batch_strands(DevCall& call, const char* what, const uint8_t* src, size_t total_bytes, const uint32_t* offs,
                        uint32_t n, uint32_t strands, StagedBatch& b);

#pragma GCC visibility pop
