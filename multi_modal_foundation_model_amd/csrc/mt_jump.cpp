// Jump-ahead for MT19937, the engine behind torch's CPU generator (host only: no HIP call, no device needed).
//
// The masker's reference-exact stream (models/masker.py) draws three [B, T, N] tensors whose values the embd-masking path
// throws away; all that survives is the generator having moved on by 3*B*T*N outputs.  MT19937 is linear over GF(2), so
// that move needs no draw:
//   * the raw (untempered) words x[j] satisfy, bit for bit, a linear recurrence whose characteristic polynomial phi has
//     degree 19937; phi is found once per process with Berlekamp-Massey over 2 * 19937 values of one output bit;
//   * x[j + e] = sum over the set bits i of g = t^e mod phi of x[j + i], for every j;
//   * torch's engine regenerates its 624 words in place, so its array is always an aligned block of x; moving D blocks on is
//     g = t^(624 D) mod phi applied to the 19937 + 623 words that the plain recurrence gives from the current block.
// A seed-initialised block is no part of the sequence (the low 31 bits of its word 0 are never read), so every jump first
// regenerates at least one block for real; the words handed to the polynomial are then always recurrence output.
#include <stdint.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/mmfm.h"

int mmfm_set_error(int code, const char* fmt, ...);

namespace {

constexpr int MT_N = 624, MT_M = 397, DEG = 19937;
constexpr uint32_t MATRIX_A = 0x9908b0dfu, UPPER = 0x80000000u, LOWER = 0x7fffffffu;
constexpr int PW = (2 * DEG + 63) / 64;                 // words of a polynomial of degree < 2 * DEG
// below this many whole blocks the generator is simply stepped: a jump costs 19937 + 623 recurrence steps plus ~10^4 XORs of a
// 624-word block (about what 2000 regenerations cost), and a new block count costs one t^e mod phi on top
constexpr uint64_t JUMP_MIN_BLOCKS = 2048;
constexpr size_t G_CACHE_MAX = 32;

inline uint32_t twist(uint32_t hi, uint32_t lo) {
    uint32_t y = (hi & UPPER) | (lo & LOWER);
    return (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
}

// x[0..623] is a block; appends x[624..count-1] by the plain recurrence
void extend(uint32_t* x, int count) {
    for (int j = MT_N; j < count; j++) x[j] = x[j - MT_N + MT_M] ^ twist(x[j - MT_N], x[j - MT_N + 1]);
}

// one in-place regeneration, the same 624 words as MT19937RNGEngine::next_state()
void regenerate(uint32_t* s) {
    int k = 0;
    for (; k < MT_N - MT_M; k++) s[k] = s[k + MT_M] ^ twist(s[k], s[k + 1]);
    for (; k < MT_N - 1; k++) s[k] = s[k + MT_M - MT_N] ^ twist(s[k], s[k + 1]);
    s[MT_N - 1] = s[MT_M - 1] ^ twist(s[MT_N - 1], s[0]);
}

struct Cache {
    std::mutex mu;
    std::vector<int> phi;                                // exponents of phi below DEG (t^DEG itself is implied); empty: not computed
    std::map<uint64_t, std::vector<int>> g;              // block count D -> set bits of t^(624 D) mod phi
};
Cache& cache() {
    static Cache c;
    return c;
}

// Berlekamp-Massey over GF(2), bit-packed.  `win` bit i holds s[n - i], so the discrepancy is parity(conn & win).
bool find_phi(std::vector<int>& phi) {
    const int NBITS = 2 * DEG, W = (DEG + 1 + 63) / 64 + 1;
    std::vector<uint32_t> x(MT_N + NBITS);
    x[0] = 19650218u;
    for (int j = 1; j < MT_N; j++) x[j] = 1812433253u * (x[j - 1] ^ (x[j - 1] >> 30)) + (uint32_t)j;
    extend(x.data(), MT_N + NBITS);                      // s[n] = bit 0 of x[624 + n]: recurrence output only
    std::vector<uint64_t> conn(W, 0), prev(W, 0), tmp(W), win(W, 0);
    conn[0] = prev[0] = 1;
    int L = 0, m = 1;
    for (int n = 0; n < NBITS; n++) {
        uint64_t carry = x[MT_N + n] & 1u;
        for (int w = 0; w < W; w++) {
            uint64_t v = win[w];
            win[w] = (v << 1) | carry;
            carry = v >> 63;
        }
        uint64_t acc = 0;
        const int used = L / 64 + 1;
        for (int w = 0; w < used; w++) acc ^= conn[w] & win[w];
        if (!(__builtin_popcountll(acc) & 1)) {
            m++;
            continue;
        }
        const bool grow = 2 * L <= n;
        if (grow) tmp = conn;
        const int ws = m / 64, bs = m % 64;               // conn ^= prev << m
        for (int w = W - 1; w >= ws; w--) {
            uint64_t v = prev[w - ws] << bs;
            if (bs && w - ws - 1 >= 0) v |= prev[w - ws - 1] >> (64 - bs);
            conn[w] ^= v;
        }
        if (grow) {
            L = n + 1 - L;
            prev.swap(tmp);
            m = 1;
        } else {
            m++;
        }
    }
    if (L != DEG) return false;
    // conn(x) = sum c_i x^i with s[n] = sum_{i >= 1} c_i s[n - i]; the characteristic polynomial is its reciprocal
    phi.clear();
    for (int i = 1; i <= DEG; i++)
        if ((conn[i / 64] >> (i % 64)) & 1) phi.push_back(DEG - i);
    return !phi.empty();
}

inline void flip(uint64_t* p, int bit) { p[bit >> 6] ^= 1ull << (bit & 63); }
inline bool test(const uint64_t* p, int bit) { return (p[bit >> 6] >> (bit & 63)) & 1; }

// p has degree <= top; reduce it below DEG modulo phi (phi is sparse: one flip per term and set high bit)
void reduce(uint64_t* p, int top, const std::vector<int>& phi) {
    for (int b = top; b >= DEG; b--)
        if (test(p, b)) {
            flip(p, b);
            for (int e : phi) flip(p, e + b - DEG);
        }
}

// set bits of t^e mod phi, by left-to-right square-and-multiply
std::vector<int> power_of_t(uint64_t e, const std::vector<int>& phi) {
    std::vector<uint64_t> r(PW, 0), sq(PW);
    r[0] = 1;
    for (int bit = 63 - __builtin_clzll(e | 1); bit >= 0; bit--) {
        std::fill(sq.begin(), sq.end(), 0);
        for (int i = 0; i < DEG; i++)
            if (test(r.data(), i)) flip(sq.data(), 2 * i);
        reduce(sq.data(), 2 * DEG - 2, phi);
        if ((e >> bit) & 1) {                             // times t
            uint64_t carry = 0;
            for (int w = 0; w <= DEG / 64; w++) {
                uint64_t v = sq[w];
                sq[w] = (v << 1) | carry;
                carry = v >> 63;
            }
            reduce(sq.data(), DEG, phi);
        }
        r.swap(sq);
    }
    std::vector<int> bits;
    for (int i = 0; i < DEG; i++)
        if (test(r.data(), i)) bits.push_back(i);
    return bits;
}

// a copy of the set bits of t^(624 D) mod phi, computed on first use
bool jump_poly(uint64_t D, std::vector<int>& out) {
    Cache& c = cache();
    std::lock_guard<std::mutex> lock(c.mu);
    if (c.phi.empty() && !find_phi(c.phi)) return false;
    auto it = c.g.find(D);
    if (it == c.g.end()) {
        if (c.g.size() >= G_CACHE_MAX) c.g.clear();
        it = c.g.emplace(D, power_of_t(D * (uint64_t)MT_N, c.phi)).first;
    }
    out = it->second;
    return true;
}

}  // namespace

// Internal (C++ linkage, mt_device.hip): the set bits of t^(624 D) mod phi as 16-bit positions, ascending, from the cache above - the
// table a device-side jump of D blocks uploads once.  false: phi could not be found.
bool mmfm_mt_jump_bits(uint64_t D, std::vector<uint16_t>& out) {
    std::vector<int> g;
    if (!jump_poly(D, g)) return false;
    out.assign(g.begin(), g.end());                       // every position is below 19937
    return true;
}

extern "C" int mmfm_mt19937_jump(uint32_t* state624, int32_t* consumed, uint64_t n) {
    if (!state624 || !consumed) return mmfm_set_error(-1, "mmfm_mt19937_jump: null argument");
    if (*consumed < 0 || *consumed > MT_N) return mmfm_set_error(-1, "mmfm_mt19937_jump: consumed = %d is outside 0..624", (int)*consumed);
    if (n > (1ull << 62)) return mmfm_set_error(-1, "mmfm_mt19937_jump: n is out of range");
    const uint64_t total = (uint64_t)*consumed + n;
    if (total <= (uint64_t)MT_N) {                        // stays inside the current block
        *consumed = (int32_t)total;
        return 0;
    }
    uint64_t d = (total - 1) / MT_N;                      // regenerations that n outputs cross (>= 1 here)
    const int32_t left_over = (int32_t)(total - d * MT_N);   // 1..624 words of the last block handed out
    // whole blocks to jump: n / 624 - 2 is d - 1, d - 2 or d - 3 wherever in its block the call starts, so one n needs one g, and
    // between one and three regenerations are always real
    uint64_t D = n / MT_N >= 2 ? n / MT_N - 2 : 0;
    if (D < JUMP_MIN_BLOCKS) D = 0;
    for (uint64_t i = D; i < d; i++) {
        regenerate(state624);
        if (D && i == D) {                                // the first real block is in place: jump D blocks from it
            std::vector<int> g;
            if (!jump_poly(D, g)) return mmfm_set_error(-1, "mmfm_mt19937_jump: the characteristic polynomial has degree != 19937");
            std::vector<uint32_t> x(DEG + MT_N - 1);
            memcpy(x.data(), state624, MT_N * sizeof(uint32_t));
            extend(x.data(), DEG + MT_N - 1);
            uint32_t acc[MT_N] = {0};
            for (int b : g) {
                const uint32_t* src = x.data() + b;
                for (int k = 0; k < MT_N; k++) acc[k] ^= src[k];
            }
            memcpy(state624, acc, sizeof(acc));
        }
    }
    *consumed = left_over;
    return 0;
}

extern "C" int mmfm_mt19937_jump_reset(void) {
    Cache& c = cache();
    std::lock_guard<std::mutex> lock(c.mu);
    c.phi.clear();
    c.g.clear();
    return 0;
}
