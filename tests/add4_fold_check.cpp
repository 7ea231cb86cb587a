// Host check of the sieve's four-row fold (Two::add4 in datasketch_amd/csrc/minhash_kernels.hip) against four Two::add calls.
// A re-statement with plain C++ stand-ins for v_min3_u32 / v_med3_u32, not the kernel's code: it shows that the identity
//     L = min3(x1, x2, x3), Mi = med3(x1, x2, x3), t = med3(k1, L, x4), k1 = min3(k1, L, x4), k2 = min3(k2, Mi, t)
// yields the two smallest of {k1, k2, x1, x2, x3, x4} as a multiset -- equal values and the 2^32-1 a record starts from
// included.  That the kernel computes the same is what tests/test_gpu_sieve_row_groups.py checks on the device.
//
//     c++ -O1 -g -fsanitize=address,undefined tests/add4_fold_check.cpp -o add4_fold_check && ./add4_fold_check
// (run by tests/test_sieve_row_groups_host.py).  Exit status 0 and "ok <cases>" on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace {

constexpr uint32_t kMaxHash = 0xFFFFFFFFu;

uint32_t umin3(uint32_t x, uint32_t y, uint32_t z) { return std::min(std::min(x, y), z); }
uint32_t umed3(uint32_t x, uint32_t y, uint32_t z) { return std::max(std::min(x, y), std::min(std::max(x, y), z)); }

struct Two {
    uint32_t k1 = kMaxHash, k2 = kMaxHash;
    void add(uint32_t key) {
        k2 = umed3(k1, k2, key);
        k1 = std::min(k1, key);
    }
    void add4(uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4) {
        const uint32_t L = umin3(x1, x2, x3), Mi = umed3(x1, x2, x3);
        const uint32_t t = umed3(k1, L, x4);
        k1 = umin3(k1, L, x4);
        k2 = umin3(k2, Mi, t);
    }
};

uint64_t state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// one value of a sextuple: `kind` picks the range -- full 32 bits, a handful of small values (ties everywhere), tagged keys
// (low four bits = a row number below a shared base) or the extremes
uint32_t draw(int kind) {
    const uint32_t r = next_u32();
    switch (kind) {
        case 0: return r;
        case 1: return r % 5u;
        case 2: return (1000u + (r >> 4) % 3u * 16u) | (r & 15u);
        default: return (r & 3u) == 0 ? kMaxHash : (r & 3u) == 1 ? 0u : (r & 3u) == 2 ? kMaxHash - 1u : r;
    }
}

bool check(uint32_t k1, uint32_t k2, const uint32_t (&x)[4]) {
    Two one, four;
    one.k1 = four.k1 = std::min(k1, k2);  // a record always has k1 <= k2
    one.k2 = four.k2 = std::max(k1, k2);
    for (uint32_t v : x) one.add(v);
    four.add4(x[0], x[1], x[2], x[3]);
    uint32_t all[6] = {k1, k2, x[0], x[1], x[2], x[3]};
    std::sort(all, all + 6);
    if (one.k1 != four.k1 || one.k2 != four.k2 || four.k1 != all[0] || four.k2 != all[1]) {
        std::printf("MISMATCH record (%u, %u) + {%u, %u, %u, %u}: add x4 -> (%u, %u), add4 -> (%u, %u), sorted -> (%u, %u)\n", k1, k2, x[0],
                    x[1], x[2], x[3], one.k1, one.k2, four.k1, four.k2, all[0], all[1]);
        return false;
    }
    return true;
}

}  // namespace

int main() {
    long cases = 0;
    // every sextuple over {0, 1, 2, 2^32-1}: all orders and all ties
    const uint32_t small[4] = {0u, 1u, 2u, kMaxHash};
    for (int i = 0; i < 4096; ++i) {
        const uint32_t x[4] = {small[(i >> 4) & 3], small[(i >> 6) & 3], small[(i >> 8) & 3], small[(i >> 10) & 3]};
        if (!check(small[i & 3], small[(i >> 2) & 3], x)) return 1;
        ++cases;
    }
    // a fresh record (2^32-1, 2^32-1) and 10^6 random sextuples, a quarter from each range
    for (int i = 0; i < 1000000; ++i) {
        const int kind = i & 3;
        const uint32_t x[4] = {draw(kind), draw(kind), draw(kind), draw(kind)};
        const bool fresh = (i & 63) == 4;
        if (!check(fresh ? kMaxHash : draw(kind), fresh ? kMaxHash : draw(kind), x)) return 1;
        ++cases;
    }
    // a block of 16 rows folded four at a time, and 4 + 3 (a group and the one-row remainder), against the one-row fold
    for (int i = 0; i < 100000; ++i) {
        uint32_t key[16];
        for (int r = 0; r < 16; ++r) key[r] = (draw(i & 3) & ~15u) | (uint32_t)r;
        for (int rows : {16, 7}) {
            Two one, grouped;
            int r = 0;
            for (; r + 4 <= rows; r += 4) grouped.add4(key[r], key[r + 1], key[r + 2], key[r + 3]);
            for (; r < rows; ++r) grouped.add(key[r]);
            for (r = 0; r < rows; ++r) one.add(key[r]);
            if (one.k1 != grouped.k1 || one.k2 != grouped.k2) {
                std::printf("MISMATCH block %d rows=%d: (%u, %u) against (%u, %u)\n", i, rows, one.k1, one.k2, grouped.k1, grouped.k2);
                return 1;
            }
            ++cases;
        }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
