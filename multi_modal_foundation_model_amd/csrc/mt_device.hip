// MT19937 on the device (MMFM_MT_DEVICE): the masker's corruption draws whose values are read, bit for bit as torch's CPU generator.
//
// One workgroup owns one run of whole 624-word blocks.  It holds its block in LDS and regenerates it in place in three phases
// (k < 227, 227 <= k < 454, 454 <= k <= 623: each reads only words that earlier phases wrote or that are still old), one lane per
// word, every lane reading its neighbour's old word before any lane writes.  The tempered words of the previous and of the current
// block stay in LDS, so a run may start anywhere inside a block: element j of a round reads word off + j of the pair.
// The state at the start of run s is a jump of s * P blocks, and a jump is a GF(2) convolution (mt_jump.cpp): the block is extended
// to 19937 + 623 raw words by the plain recurrence (82 KB of LDS) and every word of the new block is the XOR of the ~10^4 words that
// the set bits of t^(624 D) mod phi select.  The jumps run as a doubling tree: level k gives runs [2^k, 2^(k+1)) their states from
// runs [0, 2^k) with the polynomial of P * 2^k blocks, one launch per level, JSPLIT workgroups per jump (each extends the block itself
// and XORs a quarter of the words).  mmfm_mt_corrupt carries three states per run (the draws start BTN outputs apart); their first
// states come from the root by the polynomials of floor(BTN / 624) and floor(2 BTN / 624) blocks, the remainders ride in `off`.
#include "common.h"

#include <string.h>

#include <map>
#include <mutex>
#include <utility>
#include <vector>

bool mmfm_mt_jump_bits(uint64_t D, std::vector<uint16_t>& out);          // mt_jump.cpp

namespace {

constexpr int MT_N = 624, MT_M = 397, MT_DEG = 19937;
constexpr uint32_t MATRIX_A = 0x9908b0dfu, UPPER = 0x80000000u, LOWER = 0x7fffffffu;
constexpr int GEN_THREADS = 640;                   // 624 word lanes + 16 idle: ten whole waves
constexpr int XLEN = MT_DEG + MT_N - 1;            // raw words a jump reads
constexpr int JUMP_THREADS = 1024, JUMP_WAVES = 16;
constexpr int JSPLIT = 4, KW = MT_N / JSPLIT, KACC = (KW + 63) / 64, KPAD = KACC * 64;   // 156 words per workgroup, 3 per lane
constexpr int POLY_MAX = 19968;                    // uint16 slots of LDS behind x[]
constexpr size_t JUMP_LDS = (size_t)XLEN * 4 + (size_t)POLY_MAX * 2;
// the library's choice: at least 64 blocks a run, at most one run per CU.  A run costs a jump (4 workgroups of ~10^4 LDS reads a lane,
// about 2 us of the chip per run and draw) and saves stepping; measured at the B = 1024 masker call (profiles/masker_device.json):
// 128 / 256 / 512 / 1024 runs = 3.1 / 2.5 / 2.9 / 4.7 ms
constexpr int AUTO_BLOCKS_PER_STREAM = 64, AUTO_MAX_STREAMS = 256;

struct MtRoot { uint32_t w[MT_N]; };

__host__ __device__ __forceinline__ uint32_t twist(uint32_t hi, uint32_t lo) {
    const uint32_t y = (hi & UPPER) | (lo & LOWER);
    return (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
}
__device__ __forceinline__ uint32_t temper24(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y & 0xFFFFFFu;
}
__device__ __forceinline__ float unit24(uint32_t v) { return (float)v * 0x1p-24f; }      // exact: 24 bits

__global__ void mt_root_kernel(MtRoot root, uint32_t* states) {
    for (int k = threadIdx.x; k < MT_N; k += blockDim.x) states[k] = root.w[k];
}

// ------------------------------------------------------------------------------------------------------------------ the jumps
struct JumpArgs {
    uint32_t* states;                    // [nd][S][624]
    int S;
    int draws;                           // 0: tree level - (d, s) <- (d, s - lo) for s in [lo, lo + cnt), poly[0];  1: (d, 0) <- (0, 0), d = 1 + job, poly[d]
    int lo, cnt;
    const uint16_t* poly[3];
    int plen[3];                         // 0: a jump of no block - the copy
};

__global__ __launch_bounds__(JUMP_THREADS) void mt_jump_kernel(JumpArgs j) {
    extern __shared__ uint32_t x[];                                      // XLEN raw words, then the polynomial's bit positions
    uint16_t* pl = reinterpret_cast<uint16_t*>(x + XLEN);
    const int t = threadIdx.x, job = blockIdx.x / JSPLIT, k0 = (blockIdx.x % JSPLIT) * KW;
    int d, sdst, dsrc, ssrc, pi;
    if (j.draws) { d = job + 1; sdst = 0; dsrc = 0; ssrc = 0; pi = d; }
    else { d = job / j.cnt; sdst = j.lo + job % j.cnt; dsrc = d; ssrc = sdst - j.lo; pi = 0; }
    const uint32_t* src = j.states + ((size_t)dsrc * j.S + ssrc) * MT_N;
    uint32_t* dst = j.states + ((size_t)d * j.S + sdst) * MT_N;
    const int len = j.plen[pi];
    if (len == 0) {
        if (t < KW) dst[k0 + t] = src[k0 + t];
        return;
    }
    const uint16_t* poly = j.poly[pi];
    for (int i = t; i < len; i += JUMP_THREADS) pl[i] = poly[i];
    if (t < MT_N) x[t] = src[t];
    __syncthreads();
    for (int base = MT_N; base < XLEN; base += MT_N - MT_M) {            // 227 words a round: x[i] needs x[i - 227]
        const int i = base + t;
        if (t < MT_N - MT_M && i < XLEN) x[i] = x[i - (MT_N - MT_M)] ^ twist(x[i - MT_N], x[i - MT_N + 1]);
        __syncthreads();
    }
    const int w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63;
    uint32_t acc[KACC];
#pragma unroll
    for (int m = 0; m < KACC; m++) acc[m] = 0;
#pragma unroll 4
    for (int i = w; i < len; i += JUMP_WAVES) {                           // wave w takes every 16th set bit
        const uint32_t* xs = x + pl[i] + k0 + l;                          // pl[i] + k0 + l + 64 m <= 19936 + 623 < XLEN
#pragma unroll
        for (int m = 0; m < KACC; m++)
            if (l + 64 * m < KW) acc[m] ^= xs[64 * m];
    }
    __syncthreads();                                                      // x is read out: its head becomes the partial words
#pragma unroll
    for (int m = 0; m < KACC; m++) x[w * KPAD + l + 64 * m] = acc[m];
    __syncthreads();
    if (t < KW) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < JUMP_WAVES; q++) v ^= x[q * KPAD + t];
        dst[k0 + t] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the runs
// One regeneration of the draws in `mask`: a[d] is this lane's word of s[d] on entry (s visible to all lanes) and on return.
template <int ND>
__device__ __forceinline__ void mt_regen(uint32_t (*s)[MT_N], uint32_t (&a)[ND], int t, int mask) {
    uint32_t tw[ND];
#pragma unroll
    for (int d = 0; d < ND; d++) tw[d] = (t < MT_N - 1) ? twist(a[d], s[d][t + 1]) : 0u;      // MT_N - 1 .. 639 read nothing
    __syncthreads();
    if (t < MT_N - MT_M) {
#pragma unroll
        for (int d = 0; d < ND; d++)
            if ((mask >> d) & 1) s[d][t] = a[d] = s[d][t + MT_M] ^ tw[d];
    }
    __syncthreads();
    if (t >= MT_N - MT_M && t < 2 * (MT_N - MT_M)) {
#pragma unroll
        for (int d = 0; d < ND; d++)
            if ((mask >> d) & 1) s[d][t] = a[d] = s[d][t - (MT_N - MT_M)] ^ tw[d];
    }
    __syncthreads();
    if (t >= 2 * (MT_N - MT_M) && t < MT_N - 1) {
#pragma unroll
        for (int d = 0; d < ND; d++)
            if ((mask >> d) & 1) s[d][t] = a[d] = s[d][t - (MT_N - MT_M)] ^ tw[d];
    } else if (t == MT_N - 1) {
#pragma unroll
        for (int d = 0; d < ND; d++)
            if ((mask >> d) & 1) s[d][t] = a[d] = s[d][MT_M - 1] ^ twist(a[d], s[d][0]);
    }
    __syncthreads();
}

// (max, any NaN) over the workgroup, every lane gets the result: NaN if any, as torch.max
__device__ __forceinline__ float block_max_nan(float mx, bool nan, float* red, int t) {
    mx = wave_max(mx);
    const bool wn = __ballot(nan) != 0;
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = wn ? __int_as_float(0x7fc00000) : mx;
    __syncthreads();
    float r = -INFINITY;
    bool rn = false;
    for (int q = 0; q < GEN_THREADS / 64; q++) {
        const float v = red[q];
        if (v != v) rn = true; else r = fmaxf(r, v);
    }
    return rn ? __int_as_float(0x7fc00000) : r;
}

enum { GEN_UNIFORM = 0, GEN_BERNOULLI = 1, GEN_MAX = 2, GEN_CORRUPT = 3 };

struct GenArgs {
    const uint32_t* states;              // [nd][S][624]
    int S;
    long long P;                         // blocks per run
    unsigned long long n;                // elements
    int off[3];                          // word of the first element inside the run's first block pair, 0 .. 1246
    float p0, p1;                        // bernoulli p / zero_ratio, random_ratio
    void* out;                           // fp32 (uniform, corrupt) / uint8 (bernoulli)
    const float* src;
    const uint8_t* cm;
    long long sb, st, sn;
    int T, N;
    float* partial;                      // [S] per-run maxima (GEN_MAX writes, GEN_CORRUPT reads when use_max)
    int use_max;
};

template <int ND, int MODE>
__global__ __launch_bounds__(GEN_THREADS) void mt_gen_kernel(GenArgs g) {
    __shared__ uint32_t s[ND][MT_N];
    __shared__ uint32_t buf[ND][2][MT_N];
    __shared__ float red[GEN_THREADS / 64];
    const int t = threadIdx.x, run = blockIdx.x;
    const unsigned long long e0 = (unsigned long long)run * (unsigned long long)g.P * MT_N;
    if (e0 >= g.n) {                                                      // a trailing empty run (uniform over the workgroup)
        if (MODE == GEN_MAX && t == 0) g.partial[run] = -INFINITY;
        return;
    }
    const unsigned long long left = g.n - e0, span = (unsigned long long)g.P * MT_N;
    const unsigned long long cnt = left < span ? left : span;

    float m = 0.f;
    if (MODE == GEN_CORRUPT && g.use_max) {
        float mx = -INFINITY;
        bool nan = false;
        for (int i = t; i < g.S; i += GEN_THREADS) {
            const float v = g.partial[i];
            if (v != v) nan = true; else mx = fmaxf(mx, v);
        }
        m = block_max_nan(mx, nan, red, t);
    }

    uint32_t a[ND];
    int off[ND], step = 0;
#pragma unroll
    for (int d = 0; d < ND; d++) {
        off[d] = g.off[d];
        a[d] = 0;
        if (t < MT_N) s[d][t] = a[d] = g.states[((size_t)d * g.S + run) * MT_N + t];
        if (off[d] >= MT_N) { step |= 1 << d; off[d] -= MT_N; }
    }
    __syncthreads();
    if (step) mt_regen<ND>(s, a, t, step);
    if (t < MT_N) {
#pragma unroll
        for (int d = 0; d < ND; d++) buf[d][0][t] = temper24(a[d]);
    }

    float mx = -INFINITY;
    bool nan = false;
    for (unsigned long long r0 = 0, r = 0; r0 < cnt; r0 += MT_N, r++) {
        const int cur = (int)((r + 1) & 1);
        mt_regen<ND>(s, a, t, (1 << ND) - 1);
        if (t < MT_N) {
#pragma unroll
            for (int d = 0; d < ND; d++) buf[d][cur][t] = temper24(a[d]);
        }
        __syncthreads();
        if (t < MT_N && r0 + t < cnt) {
            const unsigned long long e = e0 + r0 + t;
            float u[ND];
#pragma unroll
            for (int d = 0; d < ND; d++) {
                const int i = off[d] + t;
                u[d] = unit24(i < MT_N ? buf[d][cur ^ 1][i] : buf[d][cur][i - MT_N]);
            }
            if constexpr (MODE == GEN_UNIFORM) {
                reinterpret_cast<float*>(g.out)[e] = u[0];
            } else if constexpr (MODE == GEN_BERNOULLI) {
                reinterpret_cast<uint8_t*>(g.out)[e] = u[0] < g.p0 ? 1 : 0;
            } else {
                const uint32_t e32 = (uint32_t)e, row = e32 / (uint32_t)g.N, nn = e32 - row * (uint32_t)g.N;
                const uint32_t b = row / (uint32_t)g.T, tt = row - b * (uint32_t)g.T;
                const bool c = g.cm[(long long)b * g.sb + (long long)tt * g.st + (long long)nn * g.sn] != 0;
                float v = g.src[e];
                const bool z = c && u[0] < g.p0;
                if (z) v = 0.f;
                if constexpr (MODE == GEN_MAX) {
                    if (v != v) nan = true; else mx = fmaxf(mx, v);
                } else {
                    if (c && !z && u[ND - 2] < g.p1) v = m * u[ND - 1];
                    reinterpret_cast<float*>(g.out)[e] = v;
                }
            }
        }
    }
    if constexpr (MODE == GEN_MAX) {
        const float r = block_max_nan(mx, nan, red, t);
        if (t == 0) g.partial[run] = r;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct Table { uint16_t* dev; int len; };
struct Tables {
    std::mutex mu;
    std::map<std::pair<int, uint64_t>, Table> t;     // (device, block count D) -> the set bits of t^(624 D) mod phi
};
Tables& tables() {
    static Tables c;
    return c;
}

// the device tables of cnt block counts (D == 0: the empty one), uploaded on first use.  Room is made before the first upload of a call,
// never between two: a table handed out earlier in the call stays valid.
int tables_of(const uint64_t* D, int cnt, int dev, Table* out, const char* who) {
    Tables& c = tables();
    std::lock_guard<std::mutex> lock(c.mu);
    size_t mine = 0, missing = 0;
    for (auto& kv : c.t) mine += kv.first.first == dev;
    for (int i = 0; i < cnt; i++) missing += D[i] != 0 && !c.t.count({dev, D[i]});
    if (missing && mine + missing > MMFM_MT_TABLES) {    // hipFree waits for the device: no launch still reads a table
        for (auto i = c.t.begin(); i != c.t.end();) {
            if (i->first.first == dev) { (void)hipFree(i->second.dev); i = c.t.erase(i); } else ++i;
        }
    }
    for (int i = 0; i < cnt; i++) {
        out[i] = Table{nullptr, 0};
        if (D[i] == 0) continue;
        auto it = c.t.find({dev, D[i]});
        if (it != c.t.end()) { out[i] = it->second; continue; }
        std::vector<uint16_t> bits;
        if (!mmfm_mt_jump_bits(D[i], bits)) return mmfm_set_error(-1, "%s: the characteristic polynomial has degree != 19937", who);
        if (bits.empty() || bits.size() > (size_t)POLY_MAX) return mmfm_set_error(-1, "%s: a polynomial of %zu terms", who, bits.size());
        Table tb{nullptr, (int)bits.size()};
        hipError_t e = hipMalloc((void**)&tb.dev, bits.size() * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMemcpy(tb.dev, bits.data(), bits.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (tb.dev) (void)hipFree(tb.dev);
            return mmfm_set_error((int)e, "%s: polynomial upload: %s", who, hipGetErrorString(e));
        }
        c.t[{dev, D[i]}] = tb;
        out[i] = tb;
    }
    return 0;
}

int plan_of(uint64_t n, int streams, int& S, int64_t& P) {
    if (n == 0 || n > (1ull << 62) || streams < 0 || streams > MMFM_MT_MAX_STREAMS) return -1;
    const uint64_t nb = (n + MT_N - 1) / MT_N;
    uint64_t s = (uint64_t)streams;
    if (streams == 0)                                   // a power of two within the bounds above: short requests step
        for (s = 1; s * 2 <= AUTO_MAX_STREAMS && s * 2 * AUTO_BLOCKS_PER_STREAM <= nb; s *= 2) {}
    if (s > nb) s = nb;
    S = (int)s;
    P = (int64_t)((nb + s - 1) / s);
    return 0;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
size_t ws_bytes_of(int S) { return align256((size_t)3 * S * MT_N * 4) + align256((size_t)S * 4); }

struct Checked {
    MtRoot root;
    int c;                               // words of root already handed out, 0 .. 623
    int S;
    int64_t P;
};

// everything that can be refused without a HIP call, then the root block: the block that holds output `skip` (a real recurrence block:
// a seed-initialised one is regenerated by the host jump), c = that output's word
int check_common(const char* who, const uint32_t* state624, int32_t consumed, uint64_t skip, uint64_t n, int streams, const void* ws,
                 int64_t ws_bytes, Checked& k) {
    MMFM_REQUIRE(state624 && ws, "%s: null pointer", who);
    MMFM_REQUIRE(consumed >= 0 && consumed <= MT_N, "%s: consumed = %d is outside 0..624", who, (int)consumed);
    MMFM_REQUIRE(n > 0 && n <= (1ull << 62) && skip <= (1ull << 62), "%s: n / skip out of range", who);
    MMFM_REQUIRE(streams >= 0 && streams <= MMFM_MT_MAX_STREAMS, "%s: streams = %d is outside 0..%d", who, streams, MMFM_MT_MAX_STREAMS);
    if (plan_of(n, streams, k.S, k.P)) return mmfm_set_error(-1, "%s: no plan", who);
    MMFM_REQUIRE(ws_bytes >= (int64_t)ws_bytes_of(k.S), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                 (long long)ws_bytes_of(k.S));
    MMFM_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace is not 16-byte aligned", who);
    return 0;
}
int make_root(const char* who, const uint32_t* state624, int32_t consumed, uint64_t skip, Checked& k) {
    memcpy(k.root.w, state624, sizeof(k.root.w));
    int32_t c = consumed;
    if (int rc = mmfm_mt19937_jump(k.root.w, &c, skip + 1)) return rc;      // one past the first output wanted: its block is in place
    k.c = c - 1;
    return 0;
}

// root -> states[0][0], the draws' first states, then the doubling tree over the runs
int launch_jumps(const char* who, const Checked& k, int nd, const uint64_t (&Q)[3], uint32_t* states, hipStream_t stream) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    int levels = 0;
    while ((1 << levels) < k.S) levels++;
    uint64_t D[2 + 16];
    Table tb[2 + 16];
    D[0] = nd > 1 ? Q[1] : 0;
    D[1] = nd > 2 ? Q[2] : 0;
    for (int q = 0; q < levels; q++) D[2 + q] = (uint64_t)k.P << q;
    if (int rc = tables_of(D, 2 + levels, dev, tb, who)) return rc;
    const Table* lv = tb + 2;
    const bool any = nd > 1;
    JumpArgs dj{};
    dj.states = states; dj.S = k.S; dj.draws = 1;
    for (int d = 1; d < nd; d++) { dj.poly[d] = tb[d - 1].dev; dj.plen[d] = tb[d - 1].len; }
    if (any || levels)
        if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(mt_jump_kernel), JUMP_LDS, who)) return rc;
    hipLaunchKernelGGL(mt_root_kernel, dim3(1), dim3(GEN_THREADS), 0, stream, k.root, states);
    if (any) hipLaunchKernelGGL(mt_jump_kernel, dim3((nd - 1) * JSPLIT), dim3(JUMP_THREADS), JUMP_LDS, stream, dj);
    for (int q = 0; q < levels; q++) {
        JumpArgs tj{};
        tj.states = states; tj.S = k.S; tj.draws = 0;
        tj.lo = 1 << q;
        tj.cnt = (k.S - tj.lo < tj.lo) ? k.S - tj.lo : tj.lo;
        tj.poly[0] = lv[q].dev; tj.plen[0] = lv[q].len;
        hipLaunchKernelGGL(mt_jump_kernel, dim3(nd * tj.cnt * JSPLIT), dim3(JUMP_THREADS), JUMP_LDS, stream, tj);
    }
    return 0;
}

bool unit_ok(float p) { return p >= 0.f && p <= 1.f; }      // false for NaN

int draw_one(const char* who, int mode, const uint32_t* state624, int32_t consumed, uint64_t skip, uint64_t n, float p, void* out,
             int streams, void* ws, int64_t ws_bytes, mmfm_stream stream) {
    Checked k;
    MMFM_REQUIRE(out, "%s: null pointer", who);
    if (mode == GEN_BERNOULLI) MMFM_REQUIRE(unit_ok(p), "%s: p = %g is outside [0, 1]", who, (double)p);
    if (int rc = check_common(who, state624, consumed, skip, n, streams, ws, ws_bytes, k)) return rc;
    if (int rc = make_root(who, state624, consumed, skip, k)) return rc;
    uint32_t* states = reinterpret_cast<uint32_t*>(ws);
    const uint64_t Q[3] = {0, 0, 0};
    hipStream_t hs = (hipStream_t)stream;
    if (int rc = launch_jumps(who, k, 1, Q, states, hs)) return rc;
    GenArgs g{};
    g.states = states; g.S = k.S; g.P = k.P; g.n = n; g.off[0] = k.c; g.p0 = p; g.out = out;
    if (mode == GEN_UNIFORM) hipLaunchKernelGGL((mt_gen_kernel<1, GEN_UNIFORM>), dim3(k.S), dim3(GEN_THREADS), 0, hs, g);
    else hipLaunchKernelGGL((mt_gen_kernel<1, GEN_BERNOULLI>), dim3(k.S), dim3(GEN_THREADS), 0, hs, g);
    MMFM_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" int mmfm_mt_plan(uint64_t n, int streams, int32_t* out_streams, int64_t* out_blocks) {
    int S;
    int64_t P;
    MMFM_REQUIRE(out_streams && out_blocks, "mmfm_mt_plan: null pointer");
    MMFM_REQUIRE(plan_of(n, streams, S, P) == 0, "mmfm_mt_plan: n = %llu, streams = %d", (unsigned long long)n, streams);
    *out_streams = S;
    *out_blocks = P;
    return 0;
}

extern "C" int64_t mmfm_mt_workspace(uint64_t n, int streams) {
    int S;
    int64_t P;
    if (plan_of(n, streams, S, P)) return mmfm_set_error(-1, "mmfm_mt_workspace: n = %llu, streams = %d", (unsigned long long)n, streams);
    return (int64_t)ws_bytes_of(S);
}

extern "C" int mmfm_mt_uniform(const uint32_t* state624, int32_t consumed, uint64_t skip, uint64_t n, float* out, int streams,
                               void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    return draw_one("mmfm_mt_uniform", GEN_UNIFORM, state624, consumed, skip, n, 0.f, out, streams, workspace, workspace_bytes, stream);
}

extern "C" int mmfm_mt_bernoulli(const uint32_t* state624, int32_t consumed, uint64_t skip, uint64_t n, float p, uint8_t* out, int streams,
                                 void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    return draw_one("mmfm_mt_bernoulli", GEN_BERNOULLI, state624, consumed, skip, n, p, out, streams, workspace, workspace_bytes, stream);
}

extern "C" int mmfm_mt_corrupt(const uint32_t* state624, int32_t consumed, int B, int T, int N, const float* src, const uint8_t* cm,
                               int64_t sb, int64_t st, int64_t sn, float zero_ratio, float random_ratio, float* dst, int streams,
                               void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    const char* who = "mmfm_mt_corrupt";
    Checked k;
    MMFM_REQUIRE(src && cm && dst, "%s: null pointer", who);
    MMFM_REQUIRE(B > 0 && T > 0 && N > 0 && (int64_t)B * T * N < (1ll << 31), "%s: bad shape [%d, %d, %d]", who, B, T, N);
    MMFM_REQUIRE(sb >= 0 && st >= 0 && sn >= 0, "%s: negative mask stride", who);
    MMFM_REQUIRE(unit_ok(zero_ratio) && unit_ok(random_ratio), "%s: zero_ratio = %g / random_ratio = %g outside [0, 1]", who,
                 (double)zero_ratio, (double)random_ratio);
    const uint64_t n = (uint64_t)B * T * N;
    if (int rc = check_common(who, state624, consumed, 0, n, streams, workspace, workspace_bytes, k)) return rc;
    if (int rc = make_root(who, state624, consumed, 0, k)) return rc;
    uint32_t* states = reinterpret_cast<uint32_t*>(workspace);
    // draw d starts d * n outputs on: Q[d] whole blocks by polynomial, the remainder (and the root's own word) in off[d] <= 623 + 623
    const uint64_t Q[3] = {0, n / MT_N, 2 * n / MT_N};
    hipStream_t hs = (hipStream_t)stream;
    if (int rc = launch_jumps(who, k, 3, Q, states, hs)) return rc;
    GenArgs g{};
    g.states = states; g.S = k.S; g.P = k.P; g.n = n;
    for (int d = 0; d < 3; d++) g.off[d] = k.c + (int)((uint64_t)d * n % MT_N);
    g.p0 = zero_ratio; g.p1 = random_ratio; g.out = dst; g.src = src; g.cm = cm;
    g.sb = sb; g.st = st; g.sn = sn; g.T = T; g.N = N;
    g.partial = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + align256((size_t)3 * k.S * MT_N * 4));
    g.use_max = (random_ratio > 0.f && zero_ratio < 1.f) ? 1 : 0;       // otherwise no element takes noise and m is never read
    if (g.use_max) hipLaunchKernelGGL((mt_gen_kernel<1, GEN_MAX>), dim3(k.S), dim3(GEN_THREADS), 0, hs, g);
    hipLaunchKernelGGL((mt_gen_kernel<3, GEN_CORRUPT>), dim3(k.S), dim3(GEN_THREADS), 0, hs, g);
    MMFM_LAUNCH_CHECK(who);
    return 0;
}
