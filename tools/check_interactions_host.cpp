// Stand-alone check of the pure-host helpers of the pair and triple passes
// (sparsepoly_amd/csrc/spfm_interactions_host.h): the pair key split, the triple key unpacking,
// the bin choice of a radix-select level and the candidate order of top-K.  Meant to be built
// with a host sanitizer:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/check_interactions_host.cpp -o check_interactions_host && \
//       ./check_interactions_host
//
// Prints "ok" and returns 0, or reports the first failed check.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../sparsepoly_amd/csrc/spfm_interactions_host.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

using namespace spfm;

static uint64_t pack(uint64_t a, uint64_t j, uint64_t l) {
    return (a << (2 * kInt3KeyBits)) | (j << kInt3KeyBits) | l;
}

int main() {
    // pair keys: both halves keep their 32 bits, at and above 2^31 - 1 too
    {
        const uint32_t edge[] = {0u, 1u, 0x7ffffffeu, 0x7fffffffu, 0x80000000u, 0xffffffffu};
        for (uint32_t r : edge)
            for (uint32_t c : edge) {
                int32_t row = 5, col = 5;
                int_split_key(((uint64_t)r << 32) | (uint64_t)c, &row, &col);
                CHECK((uint32_t)row == r && (uint32_t)col == c);
            }
        int32_t row = 0, col = 0;
        int_split_key(((uint64_t)0x7fffffffu << 32) | 0x7fffffffu, &row, &col);
        CHECK(row == INT32_MAX && col == INT32_MAX);
        int_split_key(((uint64_t)(unsigned)3000000000u << 32) | 7u, &row, &col);
        CHECK(row == (int32_t)3000000000u && col == 7);  // no bit of one half reaches the other
        // the key orders pairs by (row, col)
        CHECK((((uint64_t)1 << 32) | 0xffffffffu) < (((uint64_t)2 << 32) | 0u));
    }
    // triple keys: feature ids beyond 2^21 come out of the lookup, ids beyond d_a are refused
    {
        const int64_t da = (1 << 15) + 1;
        std::vector<int32_t> ids((size_t)da);
        for (int64_t q = 0; q < da; ++q) ids[(size_t)q] = (int32_t)(3000000 + 60000 * q);  // > 2^21
        int32_t i = -1, j = -1, l = -1;
        CHECK(int3_unpack_key(pack(0, 1, (uint64_t)da - 1), ids.data(), da, &i, &j, &l));
        CHECK(i == ids[0] && j == ids[1] && l == ids[(size_t)da - 1] && l > (1 << 21));
        CHECK(int3_unpack_key(pack(5, 700, 32000), ids.data(), da, &i, &j, &l));
        CHECK(i == ids[5] && j == ids[700] && l == ids[32000]);
        i = j = l = -1;
        CHECK(!int3_unpack_key(pack(0, 1, (uint64_t)da), ids.data(), da, &i, &j, &l));
        CHECK(!int3_unpack_key(pack((uint64_t)da, 1, 2), ids.data(), da, &i, &j, &l));
        CHECK(!int3_unpack_key(~0ull, ids.data(), da, &i, &j, &l));
        CHECK(!int3_unpack_key(0, ids.data(), 0, &i, &j, &l));
        CHECK(i == -1 && j == -1 && l == -1);  // nothing written on refusal
        // the key orders triples lexicographically
        CHECK(pack(1, 2, 3) < pack(1, 2, 4) && pack(1, 2, 32768) < pack(1, 3, 2) &&
              pack(1, 32768, 32768) < pack(2, 0, 0));
    }
    // bin choice
    {
        std::vector<uint64_t> h(4096, 0);
        int64_t tail = -1, above = -1;
        CHECK(int_select_bin(h.data(), 4096, 0, 5, &tail, &above) == -1 && tail == 0 && above == 0);
        h[10] = 3;
        h[7] = 4;
        h[0] = 100;
        CHECK(int_select_bin(h.data(), 4096, 0, 3, &tail, &above) == 10 && tail == 3 && above == 0);
        CHECK(int_select_bin(h.data(), 4096, 0, 4, &tail, &above) == 7 && tail == 7 && above == 3);
        CHECK(int_select_bin(h.data(), 4096, 2, 10, &tail, &above) == 0 && tail == 109 &&
              above == 9);
        CHECK(int_select_bin(h.data(), 4096, 0, 108, &tail, &above) == -1 && tail == 107);
        CHECK(int_select_bin(h.data(), 16, 0, 5, &tail, &above) == 7 && tail == 7);  // last level
        CHECK(int_select_bin(h.data(), 0, 1, 5, &tail, &above) == -1 && tail == 1);
    }
    // candidate order against a full sort, with ties
    {
        std::mt19937_64 rng(7);
        for (int round = 0; round < 50; ++round) {
            const size_t n = (size_t)(rng() % 300);
            std::vector<uint64_t> keys(n);
            std::vector<double> vals(n);
            for (size_t q = 0; q < n; ++q) {
                keys[q] = pack(rng() % 50, rng() % 50, rng() % 50) * 1000 + q;  // distinct
                vals[q] = (double)((long long)(rng() % 9) - 4);                  // many ties, signs
            }
            std::vector<int64_t> full(n);
            for (size_t q = 0; q < n; ++q) full[q] = (int64_t)q;
            std::sort(full.begin(), full.end(), [&](int64_t x, int64_t y) {
                const double ax = std::fabs(vals[(size_t)x]), ay = std::fabs(vals[(size_t)y]);
                return ax != ay ? ax > ay : keys[(size_t)x] < keys[(size_t)y];
            });
            for (int64_t K : {(int64_t)0, (int64_t)1, (int64_t)17, (int64_t)n, (int64_t)n + 5,
                              (int64_t)-3}) {
                std::vector<int64_t> idx;
                const int64_t nk = int_order_candidates(keys, vals, K, idx);
                CHECK(nk == std::max<int64_t>(0, std::min<int64_t>(K, (int64_t)n)));
                CHECK(idx.size() == n);
                for (int64_t q = 0; q < nk; ++q) CHECK(idx[(size_t)q] == full[(size_t)q]);
            }
        }
    }
    std::puts("ok");
    return 0;
}
