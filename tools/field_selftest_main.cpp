// The field self-test (csrc/field_selftest.hpp) as a program of its own, for a sanitizer build of the HOST forms: signed 64-bit
// overflow is what the ranges of the signed Poseidon2 are about, and UBSan sees it exactly.
//   c++ -std=c++17 -O1 -g -fsanitize=undefined,address -fno-sanitize-recover=all tools/field_selftest_main.cpp -o field_selftest
//   ./field_selftest [iterations] [table file ...]
// Runs the checks under the placeholder round constants, then under every table file: 128 + 13 canonical words in text form
// (ext_rc row by row, then int_rc), installed the way pw_set_poseidon2_constants installs them (to_monty, derive_params).
// Exit status 0, or 1 with the failing check on stderr. Header-only: nothing of the library is linked, nothing needs a GPU.
#include "../powdr_amd/csrc/field_selftest.hpp"

#include <cstdio>
#include <cstdlib>

static int run(const char* name, const p2::Params& params, uint32_t iterations) {
    const uint64_t seeds[] = {1, 2, 0xDEADBEEFull};
    for (uint64_t seed : seeds) {
        const int rc = pw::field_selftest_checks(seed, iterations, &params);
        if (rc) {
            fprintf(stderr, "%s: check %d failed (seed %llu)\n", name, rc, (unsigned long long)seed);
            return 1;
        }
    }
    printf("%s: ok\n", name);
    return 0;
}

int main(int argc, char** argv) {
    const uint32_t iterations = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 2000u;
    static p2::Params params;
    p2::generate_params(params);
    if (run("placeholder", params, iterations)) return 1;
    if (pw::field_selftest_checks(1, 1, nullptr) != 40) {
        fprintf(stderr, "a missing table must be failure 40\n");
        return 1;
    }
    for (int a = 2; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        uint32_t words[128 + 13];
        int n = 0;
        unsigned long v;
        while (n < 141 && fscanf(f, "%lu", &v) == 1 && v < bb::P) words[n++] = (uint32_t)v;
        fclose(f);
        if (n != 141) { fprintf(stderr, "%s: expected 141 canonical words\n", argv[a]); return 2; }
        params = p2::Params{};
        for (int r = 0; r < 8; ++r)
            for (int i = 0; i < 16; ++i) params.ext_rc[r][i] = bb::to_monty(words[16 * r + i]);
        for (int r = 0; r < 13; ++r) params.int_rc[r] = bb::to_monty(words[128 + r]);
        p2::derive_params(params);
        if (run(argv[a], params, iterations)) return 1;
    }
    return 0;
}
