// decodebank_plan.cpp -- what the decoder banks share on the host (csrc/hz_decodebank_plan.h, csrc/hz_received.h) as a
// stand-alone program, built by tests/test_decodebank_plan.py with AddressSanitizer and UndefinedBehaviorSanitizer:
//   1. slot_frame against plain division for every slot of rows x cap, under every kind of count and under none;
//   2. check_call under each bank's Slots: every refusal once with its exact message and code, two faults in one call
//      giving the earlier one's message, the dense banks taking overlapping and in-place pointers, and the cases of
//      tests/host/rs_plan.cpp under the Reed-Solomon bank's;
//   3. the received values: quantise at its special values and half-way cases, hard at levels 1 and 127, packed_bit.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "hz_decodebank_plan.h"
#include "hz_ldpc_plan.h"
#include "hz_received.h"
#include "hz_rs_plan.h"
#include "hz_viterbi_plan.h"

using namespace hz;

static void check_failed(int line, const char *what) {
    printf("decodebank_plan: line %d: %s\n", line, what);
    exit(1);
}
#define CHECK(c) ((c) ? (void)0 : check_failed(__LINE__, #c))

// ---- 1. slot_frame ----
static size_t slots_walked = 0, live_slots = 0;

static void slot_frames() {
    for (uint32_t R : {1u, 2u, 3u, 65u})
        for (uint32_t cap : {1u, 2u, 3u, 17u}) {
            const uint32_t kinds[6] = {0u, 1u, cap - 1, cap, cap + 5, 0xffffffffu};
            for (uint32_t shift = 0; shift <= 6; shift++) {  // shift 6: no counts
                std::vector<uint32_t> counts(R);             // (exactly R entries on the heap: a read past a row's is caught)
                for (uint32_t r = 0; r < R; r++) counts[r] = kinds[(r + shift) % 6];
                const uint32_t *c = shift < 6 ? counts.data() : nullptr;
                for (uint32_t slot = 0; slot < R * cap; slot++) {
                    uint32_t r = ~0u, f = ~0u;
                    const bool live = dbp::slot_frame(slot, cap, c, &r, &f);
                    CHECK(r == slot / cap && f == slot % cap && r < R);
                    const uint32_t cnt = c ? counts[r] : cap;
                    CHECK(live == (f < (cnt < cap ? cnt : cap)));
                    slots_walked++, live_slots += live;
                }
            }
        }
}

// ---- 2. check_call ----
static const char *const kCapWhy = "cap is at least 1 and rows * cap at most 2^22";
static const char *const kNullWhy = "null in, out or info";

struct Fault {
    std::function<void(dbp::Call &)> plant;
    unsigned fields;  // the fields of the call it touches: two faults over the same one are not combined
    int code;
    const char *why;
    bool pitched_only;
};
enum { kCap = 1, kIn = 2, kOut = 4, kInfo = 8, kIPitch = 16, kOPitch = 32, kIStride = 64, kOStride = 128 };

static size_t refusals_seen = 0, pairs_seen = 0;

// in the order of precedence
static void refusals(const dbp::Slots &s, const char *in_stride_why, const char *out_stride_why) {
    const uintptr_t A = (uintptr_t)1 << 24;
    const size_t pi = s.in_width + (s.pitched ? 4 : 0), po = s.out_width + (s.pitched ? 12 : 0), cap = 3;
    const dbp::Call good{A, 2 * A, cap * pi + 8, pi, cap * po + 16, po, cap, 2, true};
    const char *why = "?";
    CHECK(dbp::check_call(s, good, &why) == dbp::kOk && why == nullptr);
    const std::vector<Fault> faults = {
        {[](dbp::Call &c) { c.cap = 0; }, kCap, dbp::kInvalid, kCapWhy, false},
        {[](dbp::Call &c) { c.cap = dbp::kMaxFrames / 2 + 1; }, kCap, dbp::kInvalid, kCapWhy, false},
        {[](dbp::Call &c) { c.in = 0; }, kIn, dbp::kInvalid, kNullWhy, false},
        {[](dbp::Call &c) { c.out = 0; }, kOut, dbp::kInvalid, kNullWhy, false},
        {[](dbp::Call &c) { c.has_info = false; }, kInfo, dbp::kInvalid, kNullWhy, false},
        {[&](dbp::Call &c) { c.in_pitch = s.in_width - 1; }, kIPitch, dbp::kInvalid, "in_pitch is below the frame bytes", true},
        {[&](dbp::Call &c) { c.out_pitch = s.out_width - 1; }, kOPitch, dbp::kInvalid, "out_pitch is below the data bytes", true},
        {[&](dbp::Call &c) { c.in_stride = cap * pi - 1; }, kIStride, dbp::kInvalid, in_stride_why, false},
        {[&](dbp::Call &c) { c.out_stride = cap * po - 1; }, kOStride, dbp::kDstTooSmall, out_stride_why, false},
        {[](dbp::Call &c) { c.in_stride = (size_t)1 << 41; }, kIStride, dbp::kInvalid, "a pitch or stride beyond 2^40", true},
        {[](dbp::Call &c) { c.out_stride = (size_t)1 << 41; }, kOStride, dbp::kInvalid, "a pitch or stride beyond 2^40", true},
        {[](dbp::Call &c) { c.out = c.in; }, kOut, dbp::kInvalid, "in place takes equal strides and pitches", true},
        {[](dbp::Call &c) { c.out = c.in + 1; }, kOut, dbp::kInvalid, "in and out overlap in part", true},
    };
    for (size_t i = 0; i < faults.size(); i++) {
        const Fault &a = faults[i];
        dbp::Call c = good;
        a.plant(c);
        if (a.pitched_only && !s.pitched) {
            // what the Reed-Solomon bank refuses here, the dense banks take as they always did (their pitches are the widths)
            if (a.fields & (kIPitch | kOPitch)) continue;
            CHECK(dbp::check_call(s, c, &why) == dbp::kOk && why == nullptr);
            continue;
        }
        CHECK(dbp::check_call(s, c, &why) == a.code);
        CHECK(why && strcmp(why, a.why) == 0);
        refusals_seen++;
        // a later fault beside it: the earlier message
        for (size_t j = i + 1; j < faults.size(); j++) {
            const Fault &b = faults[j];
            if ((b.pitched_only && !s.pitched) || (a.fields & b.fields)) continue;
            dbp::Call d = good;
            a.plant(d), b.plant(d);
            CHECK(dbp::check_call(s, d, &why) == a.code);
            CHECK(why && strcmp(why, a.why) == 0);
            pairs_seen++;
        }
    }
    // one row: no strides
    dbp::Call one = good;
    one.rows = 1, one.in_stride = 0, one.out_stride = 0;
    CHECK(dbp::check_call(s, one, &why) == dbp::kOk);
    one.cap = dbp::kMaxFrames, one.out = (uintptr_t)1 << 44;  // (so far apart that the longest rows do not meet)
    CHECK(dbp::check_call(s, one, &why) == dbp::kOk);
    one.cap = dbp::kMaxFrames + 1;
    CHECK(dbp::check_call(s, one, &why) == dbp::kInvalid && strcmp(why, kCapWhy) == 0);
}

static void calls() {
    // the Viterbi bank: the CCSDS code over 78 data bits, hard and soft input
    vp::Config vq{vp::kBits, 7, 2, {0171, 0133, 0, 0}, 2, 3, 2, vp::kTail, 78, 1.0f, 0, 0, 0, 0};
    CHECK(!vp::check_config(vq));
    const vp::Geom vg = vp::geom(vq);
    CHECK(vg.N == 168 && vg.FB == 21 && vg.DB == 10 && vg.FB == dbp::packed_bytes(vg.N));
    const char *frames_in = "in_stride is below cap frames", *frames_out = "out_stride is below cap frames";
    refusals(dbp::dense(vg.FB, vg.DB), frames_in, frames_out);
    refusals(dbp::dense(vg.N, vg.DB), frames_in, frames_out);
    // the LDPC bank: a (7, 4) code, hard and soft input
    lp::Config lq{lp::kSoftF32, 3, 7, 12, 0, 7, 4, 1.0f, 1, 10, 12, 0};
    CHECK(!lp::check_config(lq));
    const lp::Geom lg = lp::geom(lq);
    CHECK(lg.FB == 1 && lg.DB == 1 && lg.N == 7);
    refusals(dbp::dense(lg.FB, lg.DB), frames_in, frames_out);
    refusals(dbp::dense(lg.N, lg.DB), frames_in, frames_out);
    const dbp::Slots d = dbp::dense(lg.N, lg.DB);
    CHECK(!d.pitched && strcmp(d.in_stride_why, frames_in) == 0 && strcmp(d.out_stride_why, frames_out) == 0);
    // the Reed-Solomon bank
    const rsp::Config ok{0x187, 112, 11, 32, 255, 4, 255};
    CHECK(!rsp::check_config(ok));
    const rsp::Geom g = rsp::geom(ok);  // F = 1020, I k = 892
    const dbp::Slots rs = rsp::slots(g);
    CHECK(rs.pitched && rs.in_width == 1020 && rs.out_width == 892);
    refusals(rs, "in_stride is below cap frame slots", "out_stride is below cap frame slots");
    // ... and the cases of tests/host/rs_plan.cpp
    const char *why;
    const uintptr_t A = 1 << 20;
    auto call = [&](uintptr_t in, uintptr_t out, size_t is, size_t ip, size_t os, size_t op, size_t cap, size_t rows, bool info = true) {
        const int a = dbp::check_call(rs, dbp::Call{in, out, is, ip, os, op, cap, rows, info}, &why);
        const char *through;
        CHECK(rsp::check_call(g, rsp::Call{in, out, is, ip, os, op, cap, rows, info}, &through) == a && through == why);
        return a;
    };
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kOk);
    CHECK(call(A, 2 * A, 0, 1020, 0, 892, 3, 1) == dbp::kOk);  // one row: no strides
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 0, 2) == dbp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, (dbp::kMaxFrames / 2) + 1, 2) == dbp::kInvalid);
    CHECK(call(0, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kInvalid && call(A, 0, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 3, 2, false) == dbp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1019, 3 * 892, 892, 3, 2) == dbp::kInvalid && call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 891, 3, 2) == dbp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020 - 1, 1020, 3 * 892, 892, 3, 2) == dbp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892 - 1, 892, 3, 2) == dbp::kDstTooSmall);
    CHECK(call(A, A, 3 * 1020, 1020, 3 * 1020, 1020, 3, 2) == dbp::kOk);  // in place
    CHECK(call(A, A, 3 * 1020, 1020, 3 * 1024, 1020, 3, 2) == dbp::kInvalid && call(A, A, 3 * 1024, 1024, 3 * 1024, 1020, 3, 2) == dbp::kInvalid);
    const size_t ispan = 3 * 1020 + 2 * 1020 + 1020, ospan = 3 * 892 + 2 * 892 + 892;
    CHECK(call(A, A + ispan, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kOk && call(A, A + ispan - 1, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kInvalid);
    CHECK(call(A + ospan, A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kOk && call(A + ospan - 1, A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == dbp::kInvalid);
    CHECK(call(A, A + 1, 3 * 1020, 1020, 3 * 1020, 1020, 3, 2) == dbp::kInvalid);
    CHECK(call(A, 2 * A, (size_t)1 << 41, 1020, 3 * 892, 892, 3, 2) == dbp::kInvalid && call(A, 2 * A, 0, ~(size_t)0, 0, 892, 3, 1) == dbp::kInvalid);
    // the limits and kinds are one set of values
    CHECK(vp::kMaxRows == 8192 && lp::kMaxRows == 8192 && rsp::kMaxRows == 8192);
    CHECK(vp::kMaxFrames == (size_t)1 << 22 && lp::kMaxFrames == (size_t)1 << 22 && rsp::kMaxFrames == (size_t)1 << 22);
    CHECK(vp::kBits == 1 && vp::kSoftF32 == 32 && lp::kBits == 1 && lp::kSoftF32 == 32);
    CHECK(dbp::packed_bytes(1) == 1 && dbp::packed_bytes(8) == 1 && dbp::packed_bytes(9) == 2 && dbp::packed_bytes(8192) == 1024);
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(!dbp::check_scale(1.0f) && !dbp::check_scale(FLT_MAX) && !dbp::check_scale(FLT_MIN));
    for (float bad : {0.0f, -0.0f, -1.0f, inf, -inf, std::numeric_limits<float>::quiet_NaN()})
        CHECK(dbp::check_scale(bad) && strcmp(dbp::check_scale(bad), "scale is finite and positive") == 0);
}

// ---- 3. the received values ----
static void received() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // (tests/test_viterbi_cpu.py lists the same values for the Python restatement)
    const float xs[] = {inf, -inf, nan, -0.0f, 0.5f, 1.5f, 2.5f, -0.5f, -1.5f, 126.6f, 1e30f};
    const int want[] = {127, -127, 0, 0, 0, 2, 2, 0, -2, 127, 127};
    for (size_t i = 0; i < sizeof xs / sizeof xs[0]; i++) CHECK(rx::quantise(xs[i], 1.0f) == want[i]);
    CHECK(rx::quantise(-2.5f, 1.0f) == -2 && rx::quantise(126.5f, 1.0f) == 126 && rx::quantise(-126.5f, 1.0f) == -126);
    CHECK(rx::quantise(-126.6f, 1.0f) == -127 && rx::quantise(-1e30f, 1.0f) == -127 && rx::quantise(0.0f, 1.0f) == 0);
    // the largest finite scale: products overflow to the infinities and saturate; 0 and NaN stay 0
    CHECK(rx::quantise(1.0f, FLT_MAX) == 127 && rx::quantise(-1.0f, FLT_MAX) == -127 && rx::quantise(2.0f, FLT_MAX) == 127);
    CHECK(rx::quantise(-2.0f, FLT_MAX) == -127 && rx::quantise(0.0f, FLT_MAX) == 0 && rx::quantise(-0.0f, FLT_MAX) == 0);
    CHECK(rx::quantise(nan, FLT_MAX) == 0 && rx::quantise(inf, FLT_MAX) == 127 && rx::quantise(FLT_MIN, FLT_MAX) == 4);
    CHECK(rx::quantise(0.25f, 2.0f) == 0 && rx::quantise(0.75f, 2.0f) == 2 && rx::quantise(1.0f, 0.5f) == 0);
    // both banks' spellings are these
    CHECK(vm::quantise(1.5f, 1.0f) == 2 && lm::quantise(-1.5f, 1.0f) == -2);
    CHECK(rx::hard(1, 1) == 1 && rx::hard(0, 1) == -1 && rx::hard(1, 127) == 127 && rx::hard(0, 127) == -127);
    CHECK(vm::hard(1) == 1 && vm::hard(0) == -1 && lm::hard(1, 127) == 127 && lm::hard(0, 5) == -5);
    // bits 0, 7, 8 and the last of an odd length (13 bits: exactly 2 bytes on the heap)
    std::vector<uint8_t> bytes = {0x81, 0x88};
    CHECK(rx::packed_bit(bytes.data(), 0) == 1 && rx::packed_bit(bytes.data(), 7) == 1 && rx::packed_bit(bytes.data(), 8) == 1);
    CHECK(rx::packed_bit(bytes.data(), 12) == 1 && rx::packed_bit(bytes.data(), 1) == 0 && rx::packed_bit(bytes.data(), 11) == 0);
    bytes = {0x7e, 0x77};
    CHECK(rx::packed_bit(bytes.data(), 0) == 0 && rx::packed_bit(bytes.data(), 7) == 0 && rx::packed_bit(bytes.data(), 8) == 0);
    CHECK(rx::packed_bit(bytes.data(), 12) == 0 && vm::packed_bit(bytes.data(), 1) == 1 && lm::packed_bit(bytes.data(), 11) == 1);
}

int main() {
    slot_frames();
    calls();
    received();
    printf("slots: %zu, live: %zu; refusals: %zu, pairs: %zu\n", slots_walked, live_slots, refusals_seen, pairs_seen);
    printf("decodebank_plan ok\n");
    return 0;
}
