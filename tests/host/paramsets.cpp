// paramsets.cpp -- the loop banks' parameter-set bookkeeping (csrc/hz_paramsets.h) over the AGC bank's own check and
// derivation (csrc/hz_agc_plan.h), as a stand-alone program for the sanitizers: one set against R copies of it, a
// refusal in the last row and in the first of two bad rows, and a holder left as it was by a refused call.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hz_agc_plan.h"
#include "hz_paramsets.h"

using namespace hz;

struct AgcSets {
    static constexpr size_t kParams = ap::kParams;
    static const char *check_params(const float *p) { return ap::check_params(p); }
    static am::Loop derive(const float *p) { return ap::derive(p); }
};

static int fails = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #cond);     \
            fails++;                                             \
        }                                                        \
    } while (0)

static bool same(const am::Loop &a, const am::Loop &b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
    const float loud[ap::kParams] = {0.25f, 0.5f, 0.25f, 0.2f, 1.0f, 0.5f, 2.0f};
    const float quiet[ap::kParams] = {4.0f, 0.5f, 0.5f, 0.2f, 1.0f, 0.5f, 2.0f};

    // one set, and R copies of it: the same constants R times, the caller's floats kept as given
    lb::ParamSets<am::Loop> one, many;
    CHECK(lb::stage_sets<AgcSets>(loud, 1, one) == nullptr);
    CHECK(one.params.size() == ap::kParams && one.loop.size() == 1);
    CHECK(same(one.loop[0], ap::derive(loud)));
    for (size_t R : {size_t(1), size_t(3), size_t(64), size_t(8192)}) {
        std::vector<float> p(R * ap::kParams);
        for (size_t r = 0; r < R; r++) memcpy(&p[r * ap::kParams], loud, sizeof loud);
        CHECK(lb::stage_sets<AgcSets>(p.data(), R, many) == nullptr);
        CHECK(many.params == p && many.loop.size() == R);
        for (size_t r = 0; r < R; r++) CHECK(same(many.loop[r], one.loop[0]));
    }

    // rows of their own: row r's constants are those of row r's set
    {
        const size_t R = 5;
        std::vector<float> p(R * ap::kParams);
        for (size_t r = 0; r < R; r++) memcpy(&p[r * ap::kParams], r % 2 ? quiet : loud, sizeof loud);
        CHECK(lb::stage_sets<AgcSets>(p.data(), R, many) == nullptr);
        for (size_t r = 0; r < R; r++) CHECK(same(many.loop[r], ap::derive(r % 2 ? quiet : loud)));

        // a refused last row: the refusal is that row's, and the holder keeps every bit it had
        const lb::ParamSets<am::Loop> before = many;
        std::vector<float> bad = p;
        bad[(R - 1) * ap::kParams + 1] = 0.75f;  // attack above 0.5
        const char *why = lb::stage_sets<AgcSets>(bad.data(), R, many);
        CHECK(why && strcmp(why, "0 <= attack <= 0.5") == 0);
        CHECK(many.params == before.params && many.loop.size() == before.loop.size());
        for (size_t r = 0; r < R; r++) CHECK(same(many.loop[r], before.loop[r]));
        // the same sets as ONE set are accepted: the rows behind the first are not read
        CHECK(lb::stage_sets<AgcSets>(bad.data(), 1, one) == nullptr);

        // two bad rows: the first in row order answers
        bad[1 * ap::kParams + 0] = 0.0f;  // ref below 2^-64
        why = lb::stage_sets<AgcSets>(bad.data(), R, many);
        CHECK(why && strcmp(why, "2^-64 <= ref <= 2^64") == 0);
        CHECK(many.params == before.params);
    }

    // a refusal into an empty holder leaves it empty
    {
        lb::ParamSets<am::Loop> empty;
        float nan_set[ap::kParams];
        memcpy(nan_set, loud, sizeof loud);
        nan_set[6] = NAN;
        CHECK(lb::stage_sets<AgcSets>(nan_set, 1, empty) != nullptr);
        CHECK(empty.params.empty() && empty.loop.empty());
    }

    if (fails) return 1;
    printf("paramsets ok\n");
    return 0;
}
