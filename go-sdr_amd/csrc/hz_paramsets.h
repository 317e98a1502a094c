// hz_paramsets.h -- the parameter-set bookkeeping of the loop banks (hz_loopbank.h), HIP-free so that
// tests/host/paramsets.cpp can run it under the sanitizers: one set of P::kParams floats for all rows or one per row,
// every set checked, the loop constants derived from each, and nothing of the holder touched before all of it is known
// to be good.  P: kParams, check_params(p) -> the refusal or null, derive(p) -> L.
#pragma once
#include <stddef.h>

#include <vector>

namespace hz {
namespace lb {

template <typename L> struct ParamSets {
    std::vector<float> params;  // the caller's: one set, or one per row
    std::vector<L> loop;        // derived from them, set by set
};

// `sets` sets at `params` (not null) checked and derived into `next`: the first refusal in row order, `next` as it
// was -- or null, `next` replaced.
template <class P, typename L> const char *stage_sets(const float *params, size_t sets, ParamSets<L> &next) {
    for (size_t r = 0; r < sets; r++)
        if (const char *why = P::check_params(params + r * P::kParams)) return why;
    ParamSets<L> s{std::vector<float>(params, params + sets * P::kParams), std::vector<L>(sets)};
    for (size_t r = 0; r < sets; r++) s.loop[r] = P::derive(params + r * P::kParams);
    next.params.swap(s.params);
    next.loop.swap(s.loop);
    return nullptr;
}

}  // namespace lb
}  // namespace hz
