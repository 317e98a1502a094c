// rows_plan.cpp -- csrc/hz_rows.h under AddressSanitizer + UndefinedBehaviorSanitizer, checked against expectations
// computed with Python's big integers (tests/test_rows_plan.py writes them to the file named on the command line):
//   S rows count pitch size ok elems bytes dense   a span: refused (ok = 0, the rest 0) exactly where a product or sum
//                                                  does not fit 64 bits
//   R host rows count pitch pinned route           the route: 0 nothing, 1 dense, 2 the caller's rows, 3 the 2-D copy
//   K host rows count pitch pinned route           the route where rows without a gap stay rows (dense_run = false)
// Prints "rows_plan ok".
#include <cinttypes>
#include <cstdio>

#include "hz_rows.h"

using namespace hz::rows;

static_assert(sizeof(size_t) == 8, "the expectations are for a 64-bit size_t");
static_assert(kNothing == 0 && kDense == 1 && kCaller == 2 && kCopy2D == 3, "the routes' numbers in the case file");

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    char line[256];
    long lineno = 0, spans = 0, routes = 0;
    int failures = 0;
    while (fgets(line, sizeof line, f)) {
        lineno++;
        uint64_t rows, count, pitch, size, elems, bytes, dense;
        int ok, host, pinned, want;
        char kind;
        if (sscanf(line, "S %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %" SCNu64 " %" SCNu64 " %" SCNu64, &rows, &count, &pitch, &size, &ok,
                   &elems, &bytes, &dense) == 8) {
            const Span s = span(rows, count, pitch, size);
            spans++;
            if (s.ok != (ok != 0) || s.elems != elems || s.bytes != bytes || s.dense_bytes != dense) {
                if (failures++ < 20) printf("FAIL line %ld: span ok %d elems %zu bytes %zu dense %zu\n", lineno, (int)s.ok, s.elems, s.bytes, s.dense_bytes);
            }
        } else if (sscanf(line, "%c %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d", &kind, &host, &rows, &count, &pitch, &pinned, &want) == 7 &&
                   (kind == 'R' || kind == 'K')) {
            const int got = (int)route(host != 0, rows, count, pitch, pinned != 0, kind == 'R');
            routes++;
            if (got != want && failures++ < 20) printf("FAIL line %ld: route %d\n", lineno, got);
        } else {
            printf("FAIL line %ld: not a case\n", lineno);
            failures++;
        }
    }
    fclose(f);
    printf("spans: %ld routes: %ld\n", spans, routes);
    if (failures) return 1;
    printf("rows_plan ok\n");
    return 0;
}
