// test_covar.cpp -- hzsdr::array::Covariance and hzsdr::array::Scan (go-sdr_amd/cxx/hzsdr.hpp) over the C ABI in a HOST
// context, on known answers.  Three channels carry s, i s and 2 s for a sequence s of small integers: every product and
// every sum is exact in float32, so R = sum |s|^2 * v v^H with v = (1, i, 2) is checked with ==, block by block, through
// both entries, with the open block flushed; the scan of R with w = e_k gives the diagonal and with w = (1, -i, 0) / ...
// the closed form.  Prints "covar-cxx ok" and exits 0.
#include <cstdio>
#include <cstring>

#include "go-sdr_amd/cxx/hzsdr.hpp"

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)

using cf = std::complex<float>;

int main() {
    using namespace hzsdr;
    Context ctx(0);
    const size_t N = 3, B = 700, n = 2 * B + 300;
    const cf v[N] = {{1.0f, 0.0f}, {0.0f, 1.0f}, {2.0f, 0.0f}};
    std::vector<Buffer> bufs;
    for (size_t i = 0; i < N; i++) bufs.emplace_back(HZSDR_FMT_C64, n);
    Buffer block(HZSDR_FMT_C64, N * (n + 11));  // the same rows with a pitch of n + 11
    std::vector<double> energy(3, 0.0);
    for (size_t k = 0; k < n; k++) {
        const cf s((float)((int)(k % 7) - 3), (float)((int)(k % 5) - 2));
        energy[k / B] += (double)std::norm(s);
        for (size_t i = 0; i < N; i++) {
            ((cf *)bufs[i].view.data)[k] = v[i] * s;
            ((cf *)block.view.data)[i * (n + 11) + k] = v[i] * s;
        }
    }
    array::Covariance cov(ctx, HZSDR_FMT_C64, N, B);
    CHECK(cov.Channels() == N && cov.Block() == B && cov.BlocksFor(n) == 2);
    CHECK(std::get<0>(cov.Plan()) == 256 && std::get<2>(cov.Plan()) == HZSDR_COVAR_FORM_ONE_TILE);
    std::vector<Samples> chans;
    for (auto &b : bufs) chans.push_back(b.view);
    auto r = cov.Push(chans);
    CHECK(r.size() == 2 * N * N);
    CHECK(cov.Pending() == std::make_tuple((uint64_t)n, (uint64_t)2, (size_t)300));
    const auto tail = cov.Flush();
    CHECK(tail.size() == N * N && cov.Flush().empty());
    r.insert(r.end(), tail.begin(), tail.end());
    for (size_t b = 0; b < 3; b++)
        for (size_t i = 0; i < N; i++)
            for (size_t j = 0; j < N; j++) {
                const cf want = (float)energy[b] * v[i] * std::conj(v[j]);
                CHECK(r[(b * N + i) * N + j] == want);
            }
    // the pitched entry, cut inside a segment: the same bits
    auto a = cov.PushRows(block.view.data, 301, n + 11);
    CHECK(a.empty());
    auto c = cov.PushRows((cf *)block.view.data + 301, n - 301, n + 11);
    const auto t2 = cov.Flush();
    c.insert(c.end(), t2.begin(), t2.end());
    CHECK(c.size() == r.size() && std::memcmp(c.data(), r.data(), r.size() * sizeof(cf)) == 0);
    // the scan: unit vectors read the diagonal; w = (1, 1, 1) gives energy * |sum_i conj(v_i)|^2 ... = energy * |1 - i + 2|^2
    std::vector<cf> w = {{1, 0}, {0, 0}, {0, 0}, {0, 0}, {1, 0}, {0, 0}, {0, 0}, {0, 0}, {1, 0}, {1, 0}, {1, 0}, {1, 0}};
    array::Scan scan(ctx, N, w);
    CHECK(scan.Vectors() == 4);
    const auto p = scan.Run(r);
    CHECK(p.size() == 3 * 4);
    for (size_t b = 0; b < 3; b++) {
        CHECK(p[b * 4 + 0] == (float)energy[b] && p[b * 4 + 1] == (float)energy[b] && p[b * 4 + 2] == 4.0f * (float)energy[b]);
        CHECK(p[b * 4 + 3] == 10.0f * (float)energy[b]);  // |1 + i + 2|^2 = 10
    }
    for (size_t bad : {(size_t)1, (size_t)17})
        try {
            array::Covariance x(ctx, HZSDR_FMT_C64, bad, 16);
            CHECK(!"a channel count outside 2 ... 16 accepted");
        } catch (const Error &e) {
            CHECK(e.status == HZSDR_ERR_INVALID_ARGUMENT);
        }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("covar-cxx ok\n");
    return 0;
}
