// softframe_plan.cpp -- csrc/hz_softframe_plan.h under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone:
//   1. the window test against the same inequalities in 128-bit integers: s near 0 with p0 < Kh, s + Ps at p1 and
//      p1 + 1, s + Kh at p0 and p0 - 1, positions near 2^64 (where s + Kh wraps), every h around H;
//   2. the slot arithmetic: the gather (lane by lane, float by float and pair by pair) and the carry of a push run over
//      buffers of EXACTLY the planned sizes -- HF history floats, c symbols of input -- at P = B, P = 8192 and Kh = 0,
//      with pushes of 0, 1, Kh - 1, Kh and more symbols, against a plain model that keeps the whole stream;
//   3. the maps: the float-by-float and the pair forms against q applications of (x0, x1) -> (x1, -x0);
//   4. every rejected configuration and every refused push.
// Prints "softframe_plan ok" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hz_softframe_plan.h"

using namespace hz;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint32_t wide_status(uint64_t s, uint32_t h, uint32_t H, uint64_t p0, uint64_t p1, uint32_t Kh) {
    if (h >= H) return sfp::kNoHypothesis;
    const unsigned __int128 S = s;
    return (S + Kh >= p0 && S + Kh + 1 <= p1) ? sfp::kServed : sfp::kOutside;
}

static void windows() {
    const uint32_t khs[] = {0, 1, 2, 15, 4095, 8191};
    const uint64_t p0s[] = {0, 1, 2, 14, 15, 16, 4095, 8191, 8192, 1ull << 31, (1ull << 62) - 1};
    const uint64_t cs[] = {0, 1, 2, 15, 16, 8192, 0x7ffffff0ull};
    size_t served = 0, outside = 0;
    for (uint32_t Kh : khs)
        for (uint64_t p0 : p0s)
            for (uint64_t c : cs) {
                const uint64_t p1 = p0 + c, Ps = (uint64_t)Kh + 1;
                std::vector<uint64_t> ss = {0, 1, p0, p1, p0 - Kh, p0 - Kh - 1, p0 - Kh + 1, p1 - Ps, p1 - Ps + 1, p1 - Ps - 1, ~0ull, ~0ull - Kh, ~0ull - Kh + 1,
                                            (1ull << 63), (1ull << 63) - Kh};
                for (int k = 0; k < 8; k++) ss.push_back(rnd());
                for (uint64_t s : ss)
                    for (uint32_t h = 0; h < 6; h++)
                        for (uint32_t H = 1; H <= 4; H++) {
                            const uint32_t got = sfp::window_status(s, h, H, p0, p1, Kh), want = wide_status(s, h, H, p0, p1, Kh);
                            CHECK(got == want);
                            served += got == sfp::kServed, outside += got == sfp::kOutside;
                            if (got == sfp::kServed) {
                                for (uint32_t B = 1; B <= 2; B++) {
                                    const uint64_t v0 = sfp::line_start(s, p0, Kh, B);
                                    CHECK(v0 % B == 0 && v0 + (uint64_t)Ps * B <= ((uint64_t)Kh + c) * B);
                                }
                            }
                        }
            }
    CHECK(served > 1000 && outside > 1000);
    // what the frame sync bank emits in a push passes: the payload's last symbol s + Kh lies in [p0, p1)
    for (int k = 0; k < 100000; k++) {
        const uint32_t Kh = (uint32_t)(rnd() % 8192);
        const uint64_t p0 = rnd() >> 3, c = 1 + rnd() % 100000, last = p0 + rnd() % c;
        if (last < Kh) continue;
        CHECK(sfp::window_status(last - Kh, 0, 1, p0, p0 + c, Kh) == sfp::kServed);
    }
}

struct Row {
    sfp::Config q;
    sfp::Geom g;
    std::vector<uint32_t> stream;  // every decision float so far
    std::vector<uint32_t> hist;    // exactly HF floats
    uint64_t pos = 0;
};

static uint32_t model(const Row &r, uint64_t decision_float) { return r.stream[decision_float]; }

// one push of c symbols with fresh floats; frames at every servable s are gathered both ways and compared
static void push(Row &r, uint64_t c) {
    const sfp::Config &q = r.q;
    const sfp::Geom &g = r.g;
    std::vector<uint32_t> in(c * g.sym_floats);  // exactly what the row consumes
    for (auto &v : in) v = (uint32_t)rnd();
    for (uint64_t j = 0; j < c * q.B; j++) r.stream.push_back(in[j * g.in_step]);
    const uint64_t p0 = r.pos, p1 = p0 + c;
    auto line = [&](uint64_t v) { return sfp::in_history(v, g.HF) ? r.hist.at(v) : in.at(sfp::input_float(v, g.HF, g.in_step)); };
    std::vector<uint64_t> ss = {p0 - g.Kh, p0 - g.Kh + 1, p0, p1 - g.Ps, p1 - g.Ps - 1, p0 - g.Kh - 1, p1 - g.Ps + 1};
    for (uint64_t s : ss) {
        for (uint32_t h = 0; h < q.H; h++) {
            if (sfp::window_status(s, h, q.H, p0, p1, g.Kh) != sfp::kServed) continue;
            const uint32_t map = q.maps[h];
            const uint64_t v0 = sfp::line_start(s, p0, g.Kh, q.B);
            std::vector<uint32_t> a(q.P, 0xDEADBEEFu), b(q.P, 0xDEADBEEFu);
            size_t steps = 0;
            for (uint32_t base = 0; base < q.P; base += g.step, steps++)  // a workgroup's steps, lane by lane
                for (uint32_t tid = 0; tid < sfp::kThreads; tid++) {
                    if (q.B == 2) {
                        const uint32_t k = base + 2 * tid;
                        if (k >= q.P) continue;
                        CHECK(sfp::in_history(v0 + k, g.HF) == sfp::in_history(v0 + k + 1, g.HF));  // a pair never straddles
                        uint32_t x0 = line(v0 + k), x1 = line(v0 + k + 1);
                        sfp::map_pair(x0, x1, map);
                        b.at(k) = x0, b.at(k + 1) = x1;
                    }
                    if (q.B == 1 && base + tid < q.P) b.at(base + tid) = line(v0 + base + tid) ^ sfp::map_flip(base + tid, map, 1);
                }
            CHECK(steps == (q.P + g.step - 1) / g.step);
            for (uint32_t k = 0; k < q.P; k++) a[k] = line(v0 + sfp::map_source(k, map, q.B)) ^ sfp::map_flip(k, map, q.B);
            CHECK(a == b);
            for (uint32_t k = 0; k < q.P; k++) {  // the definition: float s * B + k of the stream through the map
                const uint32_t src = sfp::map_source(k, map, q.B);
                CHECK((a[k] ^ sfp::map_flip(k, map, q.B)) == model(r, s * q.B + src));
            }
        }
    }
    if (c == 0) return;
    std::vector<uint32_t> next(g.HF);
    for (uint32_t j = 0; j < g.HF; j++) next[j] = line(sfp::carried_float(c, q.B, j));
    r.hist.swap(next);
    r.pos = p1;
    // the history is the stream's tail, zeros where it had not begun
    for (uint32_t j = 0; j < g.HF; j++) {
        const uint64_t have = r.stream.size();
        const uint32_t want = have + j >= g.HF ? r.stream[have + j - g.HF] : 0u;
        CHECK(r.hist[j] == want);
    }
}

static void slots() {
    const struct {
        int kind;
        uint32_t B, P;
    } forms[] = {{sfp::kRealF32, 1, 1},   {sfp::kC64, 1, 1},      {sfp::kC64, 2, 2},      {sfp::kRealF32, 1, 2},    {sfp::kC64, 2, 4},   {sfp::kRealF32, 1, 255},
                 {sfp::kRealF32, 1, 256}, {sfp::kRealF32, 1, 257}, {sfp::kC64, 2, 510},    {sfp::kC64, 2, 512},      {sfp::kC64, 2, 514}, {sfp::kC64, 1, 300},
                 {sfp::kRealF32, 1, 8192}, {sfp::kC64, 2, 8192},   {sfp::kC64, 1, 8192}};
    for (const auto &f : forms) {
        Row r;
        r.q = sfp::Config{f.kind, f.B, f.P, f.B == 2 ? 4u : 2u, {0, 1, f.B == 2 ? 2u : 0u, f.B == 2 ? 3u : 1u}};
        CHECK(sfp::check_config(r.q) == nullptr);
        r.g = sfp::geom(r.q);
        CHECK(r.g.Ps * f.B == f.P && r.g.Kh + 1 == r.g.Ps && r.g.HF == f.P - f.B && r.g.step == sfp::kThreads * f.B);
        CHECK(r.g.sym_floats == (f.kind == sfp::kC64 ? 2u : 1u) && r.g.in_step == (f.kind == sfp::kC64 && f.B == 1 ? 2u : 1u));
        r.hist.assign(r.g.HF, 0);
        const uint64_t Kh = r.g.Kh;
        const uint64_t cuts[] = {0, 1, 1, Kh ? Kh - 1 : 0, 0, Kh, Kh + 1, 2, 3 * Kh + 5, 1, 7, Kh / 3 + 1, Kh / 3 + 1, Kh / 3 + 1, Kh / 3 + 1, 2 * Kh + 2};
        for (uint64_t c : cuts) push(r, c);
    }
}

static void maps() {
    for (uint32_t q = 0; q < 4; q++) {
        uint32_t x0 = 0x3F800000u, x1 = 0xC0000000u, y0 = x0, y1 = x1;
        for (uint32_t k = 0; k < q; k++) {
            const uint32_t t = y0;
            y0 = y1, y1 = t ^ sfp::kSignBit;
        }
        uint32_t p0 = x0, p1 = x1;
        sfp::map_pair(p0, p1, q);
        CHECK(p0 == y0 && p1 == y1);
        const uint32_t x[2] = {x0, x1};
        CHECK((x[sfp::map_source(0, q, 2)] ^ sfp::map_flip(0, q, 2)) == y0 && (x[sfp::map_source(1, q, 2)] ^ sfp::map_flip(1, q, 2)) == y1);
        CHECK((x[sfp::map_source(6, q, 2) - 6] ^ sfp::map_flip(6, q, 2)) == y0 && (x[sfp::map_source(7, q, 2) - 6] ^ sfp::map_flip(7, q, 2)) == y1);
    }
    CHECK(sfp::map_source(5, 1, 1) == 5 && sfp::map_flip(5, 0, 1) == 0 && sfp::map_flip(5, 1, 1) == sfp::kSignBit);
    // NaN payloads, -0 and infinities: only the sign bit moves
    const uint32_t odd[] = {0x7FC12345u, 0xFF800001u, 0x80000000u, 0u, 0x7F800000u, 0xFF800000u};
    for (uint32_t v : odd) CHECK((v ^ sfp::map_flip(0, 1, 1)) == (v ^ 0x80000000u));
}

static void refusals() {
    auto cfg = [](int kind, uint32_t B, uint32_t P, uint32_t H, uint32_t m0 = 0, uint32_t m3 = 0) { return sfp::Config{kind, B, P, H, {m0, 0, 0, m3}}; };
    CHECK(!sfp::check_config(cfg(sfp::kRealF32, 1, 1, 1)) && !sfp::check_config(cfg(sfp::kC64, 2, 8192, 4, 3, 3)) && !sfp::check_config(cfg(sfp::kC64, 1, 8191, 1, 1)));
    CHECK(sfp::check_config(cfg(7, 1, 8, 1)));                 // another kind
    CHECK(sfp::check_config(cfg(sfp::kRealF32, 2, 8, 1)));     // two bits on real rows
    CHECK(sfp::check_config(cfg(sfp::kC64, 0, 8, 1)) && sfp::check_config(cfg(sfp::kC64, 3, 9, 1)));
    CHECK(sfp::check_config(cfg(sfp::kRealF32, 1, 0, 1)) && sfp::check_config(cfg(sfp::kRealF32, 1, 8193, 1)) && sfp::check_config(cfg(sfp::kC64, 2, 7, 1)));
    CHECK(sfp::check_config(cfg(sfp::kC64, 2, 0, 1)) && sfp::check_config(cfg(sfp::kC64, 2, 8194, 1)));
    CHECK(sfp::check_config(cfg(sfp::kRealF32, 1, 8, 0)) && sfp::check_config(cfg(sfp::kRealF32, 1, 8, 5)));
    CHECK(sfp::check_config(cfg(sfp::kRealF32, 1, 8, 1, 2)) && sfp::check_config(cfg(sfp::kC64, 1, 8, 4, 0, 2)) && sfp::check_config(cfg(sfp::kC64, 2, 8, 4, 0, 4)));
    CHECK(!sfp::check_config(cfg(sfp::kRealF32, 1, 8, 1, 0, 9)));  // (a map behind H is not looked at)

    const sfp::Config q = cfg(sfp::kRealF32, 1, 100, 1);
    const char *why = nullptr;
    const sfp::Call good{1000, 1000, 4, 400, 3, true, true, true, true, true, true};
    CHECK(sfp::check_call(q, good, &why) == sfp::kOk && !why);
    auto with = [&](auto change) {
        sfp::Call c = good;
        change(c);
        return sfp::check_call(q, c, &why);
    };
    CHECK(with([](sfp::Call &c) { c.out_stride = 399; }) == sfp::kDstTooSmall && why);
    CHECK(with([](sfp::Call &c) { c.out_stride = 399, c.rows = 1; }) == sfp::kOk);
    CHECK(with([](sfp::Call &c) { c.in_stride = 999; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.in_stride = 0, c.rows = 1; }) == sfp::kOk);
    CHECK(with([](sfp::Call &c) { c.cap = (1u << 22) / 3 + 1, c.out_stride = ~0ull; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.cap = (1u << 22) / 3, c.out_stride = ~0ull; }) == sfp::kOk);
    CHECK(with([](sfp::Call &c) { c.cap = ~0ull, c.out_stride = ~0ull; }) == sfp::kInvalid);  // (rows * cap wraps)
    CHECK(with([](sfp::Call &c) { c.n = c.in_stride = sfp::kMaxPush + 1; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.n = c.in_stride = sfp::kMaxPush; }) == sfp::kOk);
    CHECK(with([](sfp::Call &c) { c.has_in = false; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.has_in = false, c.n = 0; }) == sfp::kOk);
    CHECK(with([](sfp::Call &c) { c.has_positions = false; }) == sfp::kInvalid && with([](sfp::Call &c) { c.has_info = false; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.has_counts = false; }) == sfp::kInvalid && with([](sfp::Call &c) { c.has_out = false; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.has_status = false; }) == sfp::kInvalid);
    CHECK(with([](sfp::Call &c) { c.cap = 0, c.out_stride = 0, c.has_positions = c.has_info = c.has_counts = c.has_out = c.has_status = false; }) == sfp::kOk);
}

int main() {
    windows();
    slots();
    maps();
    refusals();
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("softframe_plan ok\n");
    return 0;
}
