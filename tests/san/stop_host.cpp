// The host build of the stop rule (vireo_amd/csrc/vrx_stop.h) as a stand-alone program, for a sanitizer build:
// tests/test_stop_rule_cpu.py compiles it with -fsanitize=address,undefined and runs it as a child.
//
//   stop_host CASES RESULTS
//
// CASES: { i64 n, i32 [n][4] = form, it, min_iter, max_iter, f64 [n][3] = eps, X[it - 1] as the trace holds it,
// X[it] } -- the rows of vrx_stop_verdicts.  RESULTS: { i32 verdict [n], f64 prev [n] }.  The rows live in heap
// blocks of exactly their size.  Exit status 0 unless the files cannot be read or written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../vireo_amd/csrc/vrx_stop.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: stop_host CASES RESULTS\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "stop_host: cannot open the files\n");
        return 2;
    }
    int64_t n = 0;
    if (fread(&n, sizeof n, 1, in) != 1 || n < 1 || n > (int64_t(1) << 24)) return 2;
    const size_t N = (size_t)n;
    int32_t* ri = static_cast<int32_t*>(malloc(N * 4 * sizeof(int32_t)));
    double* rd = static_cast<double*>(malloc(N * 3 * sizeof(double)));
    int32_t* verdict = static_cast<int32_t*>(malloc(N * sizeof(int32_t)));
    double* prev = static_cast<double*>(malloc(N * sizeof(double)));
    if (!ri || !rd || !verdict || !prev) return 2;
    if (fread(ri, sizeof(int32_t), N * 4, in) != N * 4 || fread(rd, sizeof(double), N * 3, in) != N * 3) return 2;
    for (size_t i = 0; i < N; ++i) {
        const int form = ri[4 * i], it = ri[4 * i + 1], min_iter = ri[4 * i + 2], max_iter = ri[4 * i + 3];
        const double eps = rd[3 * i], trace_prev = rd[3 * i + 1], cur = rd[3 * i + 2];
        prev[i] = vrx_stop_prev(it, max_iter, trace_prev, cur);
        verdict[i] = vrx_stop_judge(form, it, min_iter, max_iter, eps, prev[i], cur);
    }
    const bool ok = fwrite(verdict, sizeof(int32_t), N, out) == N && fwrite(prev, sizeof(double), N, out) == N;
    free(prev);
    free(verdict);
    free(rd);
    free(ri);
    fclose(in);
    if (fclose(out) != 0 || !ok) {
        fprintf(stderr, "stop_host: cannot write the results\n");
        return 2;
    }
    return 0;
}
