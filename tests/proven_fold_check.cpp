// Host check of the sieve's short fold (fold_proven in datasketch_amd/csrc/minhash_kernels.hip) against fold_exact.
// A re-statement in plain C++, not the kernel's code: with s = s_hi * 2^32 + s_lo, top = s >> 61, hi29 = the low 29 bits
// of s_hi and the sieve key M = lo32(s_lo + 8),
//     M >= 16   ==>   fold_exact(s) == s_lo + top   (no carry out of the low word, no Mersenne correction),
// and a listed s with M < 16 where the two differ: the guard is what makes the identity true.  That the kernel's
// finishes use the short form only under such a proof is what tests/test_gpu_sieve_finish.py checks on the device.
//
//     c++ -O1 -g -fsanitize=address,undefined tests/proven_fold_check.cpp -o proven_fold_check && ./proven_fold_check
// (run by tests/test_sieve_finish_host.py).  Exit status 0 and "ok <edge cases> <random cases>" on success.
#include <cstdint>
#include <cstdio>

namespace {

constexpr uint64_t kMersenne = (1ull << 61) - 1;

uint32_t fold_exact(uint32_t s_lo, uint32_t s_hi) {
    const uint32_t top = s_hi >> 29;
    const uint64_t y = ((((uint64_t)(s_hi & 0x1FFFFFFFu)) << 32) | s_lo) + top;
    return (uint32_t)y + (y >= kMersenne ? 1u : 0u);
}

uint32_t fold_proven(uint32_t s_lo, uint32_t s_hi) { return s_lo + (s_hi >> 29); }

// the definition, for the re-statement of fold_exact itself
uint32_t fold_reference(uint32_t s_lo, uint32_t s_hi) {
    const uint64_t s = ((uint64_t)s_hi << 32) | s_lo;
    return (uint32_t)(s % kMersenne);
}

uint32_t key_of(uint32_t s_lo) { return s_lo + 8u; }  // mod 2^32

uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bool check(uint32_t s_lo, uint32_t s_hi) {
    const uint32_t want = fold_exact(s_lo, s_hi);
    if (want != fold_reference(s_lo, s_hi)) {
        std::printf("fold_exact is not s mod p: s_lo=%u s_hi=%u\n", s_lo, s_hi);
        return false;
    }
    if (key_of(s_lo) >= 16u && fold_proven(s_lo, s_hi) != want) {
        std::printf("mismatch with M >= 16: s_lo=%u s_hi=%u exact=%u short=%u\n", s_lo, s_hi, want, fold_proven(s_lo, s_hi));
        return false;
    }
    return true;
}

}  // namespace

int main() {
    long edge = 0, random = 0, guarded_out = 0;
    // every top, the edges of hi29, s_lo within 40 of both ends of its range (keys below 16 among them: skipped by the guard)
    const uint32_t hi29_edges[] = {0u, 1u, 0x1FFFFFFEu, 0x1FFFFFFFu};
    for (uint32_t top = 0; top < 8; ++top)
        for (uint32_t hi29 : hi29_edges)
            for (int d = -40; d <= 40; ++d) {
                const uint32_t s_lo = (uint32_t)d;  // 0 .. 40 and 2^32 - 40 .. 2^32 - 1
                if (!check(s_lo, (top << 29) | hi29)) return 1;
                guarded_out += key_of(s_lo) < 16u;
                ++edge;
            }
    // the two ends of the guarded range itself: M = 16 and M = 2^32 - 1
    const uint32_t range_ends[] = {8u, 9u, 0xFFFFFFF6u, 0xFFFFFFF7u};
    for (uint32_t top = 0; top < 8; ++top)
        for (uint32_t hi29 : hi29_edges)
            for (uint32_t s_lo : range_ends) {
                if (key_of(s_lo) < 16u) return 1;
                if (!check(s_lo, (top << 29) | hi29)) return 1;
                ++edge;
            }
    while (random < 1000000) {
        const uint64_t s = next_u64();
        const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
        if (key_of(s_lo) < 16u) continue;
        if (!check(s_lo, s_hi)) return 1;
        ++random;
    }
    // The guard: M = 5 (s_lo = 2^32 - 3), top = 5 -- the sum wraps and the Mersenne correction is due.
    {
        const uint32_t s_lo = 0xFFFFFFFDu, s_hi = (5u << 29) | 0x1FFFFFFFu;
        if (key_of(s_lo) != 5u || fold_exact(s_lo, s_hi) == fold_proven(s_lo, s_hi)) {
            std::printf("the listed case with M = 5 does not differ\n");
            return 1;
        }
    }
    // and one where only the correction differs: low61(s) + top == p exactly needs s_lo + top to reach 2^32 - 1
    {
        const uint32_t s_lo = 0xFFFFFFFCu, s_hi = (3u << 29) | 0x1FFFFFFFu;  // M = 4; low61 + 3 == 2^61 - 1 == p -> 0
        if (key_of(s_lo) != 4u || fold_exact(s_lo, s_hi) != 0u || fold_proven(s_lo, s_hi) != 0xFFFFFFFFu) {
            std::printf("the listed case with M = 4 does not differ as expected\n");
            return 1;
        }
    }
    if (guarded_out == 0) return 1;
    std::printf("ok %ld %ld\n", edge, random);
    return 0;
}
