/* mmfm.h — C-ABI of libmmfm_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * masked-pretraining hot path of yzhang511/multi_modal_foundation_model.
 *
 * The reference has no FFI: the path sits behind Python classes.  Each entry
 * point below names the reference site (file:line under /root/reference/src) whose device work
 * it replaces.  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every entry returns 0 on success, a hipError_t (>0) or -1 (argument check) otherwise;
 *    the message is available through mmfm_last_error() (thread-local);
 *  - all buffers are caller-allocated DEVICE pointers; the library never allocates, frees,
 *    retains or synchronises (every launch function is hipGraph-capturable);
 *  - `stream` is a hipStream_t passed as void*;
 *  - dtype: 0 = f32 storage (parity mode), 1 = bf16 storage with fp32 accumulate/statistics;
 *  - row-major everywhere; "ld" = leading dimension in elements.
 */
#ifndef MMFM_H
#define MMFM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MMFM_VERSION 401
#define MMFM_F32 0
#define MMFM_BF16 1
/* Feature macro: bias-free linears (attention_bias / mlp_bias: false).  With it defined the NULL contracts written next to
 * mmfm_prep_entry, mmfm_rowgemm_desc, mmfm_mlp_desc, mmfm_ln_linear_grad and mmfm_sn_linear_grad hold.  No struct changed its layout and
 * no export was added, so MMFM_VERSION stays: a caller built against the earlier 401 header runs unchanged. */
#define MMFM_NULL_BIAS 1
/* Feature macro: the embedder options (embedder.act other than softsign, pos: false, bias: false).  With it defined mmfm_gemm takes the
 * act codes 12 .. 25 (mmfm_gemm_desc), mmfm_stitch_fwd a NULL pos_emb and mmfm_stitch_bwd a NULL d_pos.  No struct changed its layout and
 * no export was added: MMFM_VERSION stays, as for MMFM_NULL_BIAS. */
#define MMFM_EMBED_OPTS 1
/* Feature macro: the du-only front half of the fused MLP backward.  With it defined mmfm_mlp_bwd takes t1 == NULL && g == NULL together
 * with dx == NULL (mmfm_mlp_desc).  A library without it refuses the NULLs as an argument error; no struct changed its layout and no export
 * was added: MMFM_VERSION stays, as for MMFM_NULL_BIAS. */
#define MMFM_MLP_DX_ONLY 1
/* activation kinds of mmfm_mlp_desc.act (the fused MLP's transformer.act) */
#define MMFM_MLP_GELU 0        /* exact-erf GELU (bf16: the polynomial of act 1) */
#define MMFM_MLP_RELU 1
#define MMFM_MLP_SIGMOID 2     /* u * sigmoid(act_beta * u): silu / swish (1), quick_gelu (1.702) */
#define MMFM_MLP_GELU_TANH 3   /* gelu_new / gelu_pytorch_tanh / gelu_fast */

typedef void* mmfm_stream;

/* Counter-based dropout: keep(idx) = f(state[0], state[1], site, idx); state = 2 x uint32 in
 * DEVICE memory (so graph replays see new masks after mmfm_rng_advance).  p <= 0 disables.
 * Replaces nn.Dropout / SDPA dropout_p (mm_utils.py:52,111,114; encoder_embeddings.py:61). */
typedef struct {
    const void* state;
    uint32_t site;
    float p;
} mmfm_dropout;

int mmfm_version(void);
const char* mmfm_last_error(void);
/* 0 iff `device` is a gfx950 part. */
int mmfm_device_check(int device);
/* state[0]=lo32(mix(seed)), state[1]=step counter start */
int mmfm_rng_seed(void* state, uint64_t seed, mmfm_stream stream);
int mmfm_rng_advance(void* state, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- GEMM
 * C[m][n] = epi( sum_k A(m,k) * B(k,n) ).  Replaces every nn.Linear forward/backward on the
 * path (mm_utils.py:46-52,88-95,107-114; encoder_embeddings.py:28-30,50-54;
 * decoder_embeddings.py:83,107; mm.py:74,292) and their autograd.
 *   a_kcontig: 1 -> A(m,k) = A[m*lda + k];  0 -> A(m,k) = A[k*lda + m]
 *   b_kcontig: 1 -> B(k,n) = B[n*ldb + k] (an nn.Linear weight [N,K]);  0 -> B(k,n) = B[k*ldb + n]
 *   splits > 1: split-K; split z covers k in [z*kchunk, (z+1)*kchunk) and writes its raw fp32
 *               partial tile to C + z*slab_stride (no epilogue); reduce with mmfm_reduce_slabs.
 * epilogue (splits == 1), in this order:
 *   v = acc + bias[n]; pre_out[m*ldc+n] = v;
 *   act 1: v = gelu_erf(v)           act 2: v = softsign(v) * act_scale          (forward)
 *   act 3: v *= gelu_erf'(gradmul_pre[m*ldc+n])   act 4: v *= softsign'(gradmul_pre[..]) * act_scale
 *          (backward through the activation whose pre-activation the forward stored via pre_out);
 *   act 5: v *= (1 - |y| / act_scale)^2 * act_scale with y = gradmul_pre[..] the forward's act-2 OUTPUT: the same softsign'
 *          without a saved pre-activation (bf16 throughput mode; the fp32 parity path keeps act 4);
 *   MLP activations other than GELU (transformer.act), forward / gradient pairs; the gradient kinds multiply by f'(u),
 *   u = gradmul_pre[m*ldc+n] the pre-activation the forward stored via pre_out (as act 3):
 *   act 6: v = relu(v) = max(v, 0)                     act 7: v *= (u > 0 ? 1 : 0)
 *   act 8: v = v * sigmoid(act_scale * v)              act 9: v *= s + act_scale * u * s * (1 - s),  s = sigmoid(act_scale * u)
 *          (silu / swish: act_scale = 1;  quick_gelu: act_scale = 1.702)
 *   act 10: v = 0.5 v (1 + tanh(k (v + 0.044715 v^3))), k = sqrt(2 / pi)  (gelu_new / gelu_pytorch_tanh / gelu_fast)
 *   act 11: v *= 0.5 (1 + t) + 0.5 u (1 - t^2) k (1 + 3 * 0.044715 u^2),  t = tanh(k (u + 0.044715 u^3))
 *   Evaluated with the hardware exp / reciprocal, tanh-GELU as u * sigmoid(2 k (u + 0.044715 u^3)) (error bounds).
 *   Embedder activations (embedder.act other than softsign; MMFM_EMBED_OPTS), forward / gradient pairs.  act_scale is the embedder's
 *   `scale` in every one of them (acts 8 / 9 spend it on beta, hence the two sigmoid gates are codes of their own):
 *     forward (even)   v = f(v) * act_scale
 *     gradient (odd)   v *= f'(u) * act_scale,  u = gradmul_pre[m*ldc+n] the pre-activation the forward stored via pre_out
 *   act 12 / 13: f = identity (`identity`, `linear`); 13 reads no gradmul_pre (it may be NULL)
 *   act 14 / 15: relu                                act 16 / 17: GELU (erf in fp32, the polynomial of act 1 / 3 in bf16)
 *   act 18 / 19: v sigmoid(v) (silu / swish)         act 20 / 21: v sigmoid(1.702 v) (quick_gelu)
 *   act 22 / 23: tanh-GELU (as act 10 / 11)          act 24 / 25: tanh, f' = 1 - tanh^2
 *   The same device functions as acts 1 / 3 / 6-11; tanh as (1 - e) / (1 + e), e = exp(-2 |v|) (ranges and error bounds).
 *   Not built: gradients of tanh / relu from the activation's output (as act 5 does for softsign), sigmoid, mish, leaky_relu and the
 *   other ACT2FN names.
 *   v = dropout(v) (counter m*N+n);  v += residual[m*ldr+n];  C[m*ldc+n] = v
 */
typedef struct {
    int dtype;       /* storage of A, B, pre_out, gradmul_pre, residual and (unless c_f32) C */
    int c_f32;       /* 1: C is fp32 regardless of dtype */
    const void* A;
    const void* B;
    void* C;
    int M, N, K;
    int lda, ldb, ldc;
    int a_kcontig, b_kcontig;
    int splits, kchunk;
    int64_t slab_stride;
    const float* bias;
    void* pre_out;
    int act;
    float act_scale;
    const void* gradmul_pre;
    mmfm_dropout drop;
    const void* residual;
    int ldr;
    float* colsum;   /* optional, dtype bf16 with a_kcontig == 0 (the dW = dY^T X launches): colsum[z*slab_stride + m] =
                        sum over split z's k range of A(m,k), i.e. the bias gradient of the same nn.Linear, computed from
                        the A tiles the GEMM stages anyway (replaces a separate mmfm_colsum pass over dY).  With
                        colsum == C + M*ldc the partials sit behind each dW slab and ONE mmfm_reduce_slabs over
                        M*N + M elements finishes weight and bias gradient together. */
} mmfm_gemm_desc;
int mmfm_gemm(const mmfm_gemm_desc* d, mmfm_stream stream);
/* Two independent products, same results as two mmfm_gemm calls.  Two bf16 weight-gradient descriptors (the dY^T X form with split-K
 * slabs) run as ONE launch, each on its share of the CUs: the caller then sizes their split counts so that
 * tiles(a) * splits(a) + tiles(b) * splits(b) = 256 with the first term a multiple of 8 (mmfm_gemm_dw_tiles) - each product makes half
 * the slabs it would make alone.  The weight gradients of two linears whose dY are both at hand (MLP up / down, attention qkv / out_proj).
 * mmfm_gemm_pair_fused(a, b) says whether a pair leaves as one launch (1) or as two (0), mmfm_gemm_family which kernel each runs on alone. */
int mmfm_gemm_pair(const mmfm_gemm_desc* a, const mmfm_gemm_desc* b, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- live rows (MMFM_LIVE_ROWS)
 * The model zeroes a token of EVERY sample at each position where SAMPLE 0 is masked (mm.py:147-149, 169-171; keep0 of mmfm_mask_prep),
 * so the tokeniser rows of such a time bin are dead: nobody reads their output and their gradient is zero.  The live-bin record of one
 * modality slot says which bins are live, on the device (nothing is read back; launches keep fixed grids):
 *   rec[0]         = T_live, the number of bins t with keep0[t] != 0            (rec[1..3]: reserved, 0)
 *   rec[4 + j]     = live_t[j], the original bin of the j-th live bin, ascending (j < T_live)
 *   rec[4 + T + t] = rank[t], the place of bin t among the live bins, -1 for a dead bin
 * Dead bins are the same for every sample: row (b, t) of a [B*T] row space sits at compact row b * T_live + rank[t].
 * mmfm_live_bins: keep0 is u8 [M][T], rec int32 [M][MMFM_LIVE_REC_INTS(T)] - one record per modality slot, one launch. */
#define MMFM_LIVE_ROWS 1
#define MMFM_LIVE_REC_INTS(T) (2 * (T) + 4)
int mmfm_live_bins(const uint8_t* keep0, int T, int M, int32_t* rec, mmfm_stream stream);
/* dst[b * T_live + j][:] = src[b * T + live_t[j]][:] for rows of row_bytes bytes (a multiple of 4; 16-B accesses when rows and both
 * pointers are 16-B aligned).  Rows of dst beyond B * T_live are not written. */
int mmfm_gather_live_rows(const void* src, void* dst, int B, int T, int64_t row_bytes, const int32_t* rec, mmfm_stream stream);
/* mmfm_gemm (dtype bf16) over the compact row space of `live`.  The descriptor is the one of the full row space (B * T rows: the launch
 * geometry and the kernel choice come from it, so the grid is fixed) and the kernels read the row count B * T_live off the record:
 *   a_kcontig == 1 (x.W^T, dY.W): M = B * T_live.  Tiles beyond it exit before any load; rows of C / pre_out beyond it are not written;
 *     the dropout counter of compact row m' stays that of its original row, (m' / T_live) * T + live_t[m' % T_live], times N, plus n.
 *   a_kcontig == 0 (dY^T.X, with colsum): K = B * T_live.  The split count stays; with K_live == K the split ranges are the
 *     descriptor's, else kchunk = ceil(K_live / splits) rounded up to 64, so the live rows stay spread over all splits; a split with an
 *     empty range writes zeros for its slab and colsum. */
typedef struct {
    const int32_t* rec;   /* the record of mmfm_live_bins */
    int B, T;             /* d->M (or d->K) == B * T */
} mmfm_live_rows;
int mmfm_gemm_live(const mmfm_gemm_desc* d, const mmfm_live_rows* live, mmfm_stream stream);
/* Which kernel family mmfm_gemm (live == NULL) or mmfm_gemm_live runs for *d: one of the codes below, or a negative code with
 * mmfm_last_error set where the launch would refuse.  mmfm_gemm_pair_fused: 1 where mmfm_gemm_pair(a, b) leaves as one launch, 0 where it
 * issues a and b one after the other (each on its mmfm_gemm_family), negative where it would refuse.  Neither launches anything, reads a
 * tensor (pointers count by being NULL or not and by their alignment) or makes a HIP call: a machine without a GPU answers them.
 * MMFM_GEMM_FAMILY_F32 is the feature macro for both exports (MMFM_VERSION stays: no existing struct changed). */
#define MMFM_GEMM_FAMILY_F32 1       /* csrc/gemm.hip: fp32 */
#define MMFM_GEMM_FAMILY_TILE128 2   /* csrc/gemm_bf16.hip: bf16 MFMA, 128 x 128 tiles, every layout and epilogue */
#define MMFM_GEMM_FAMILY_BIG256 3    /* csrc/gemm_big.hip: bf16 MFMA, 256 x 256 tiles over LDS-DMA, K-contiguous operands */
#define MMFM_GEMM_FAMILY_DW128 4     /* csrc/gemm_dw.hip: the streaming weight-gradient kernel (dY^T X, fp32 out), 128-wide tiles */
#define MMFM_GEMM_FAMILY_DW256 5     /* csrc/gemm_dw.hip: the same, 256-wide tiles */
int mmfm_gemm_family(const mmfm_gemm_desc* d, const mmfm_live_rows* live_or_null);
int mmfm_gemm_pair_fused(const mmfm_gemm_desc* a, const mmfm_gemm_desc* b);

/* dst[i] (+)= sum_s src[s*slab_stride + i], fp32, deterministic order.  `src` is scratch: it may be
 * clobbered (a tall-skinny reduction first sums groups of slabs in place). */
/* Work items per K-split that a bf16 weight-gradient launch (a_kcontig == b_kcontig == 0, fp32 output, 16-B aligned rows) over K rows is
 * cut into: the caller sizes `splits` so that items x splits fills the 256 CUs once (each item writes one M-tile x N-tile fp32 slab). */
int mmfm_gemm_dw_tiles(int M, int N, int K);
int mmfm_reduce_slabs(float* dst, const float* src, int64_t n, int nslabs, int64_t slab_stride,
                      int accumulate, mmfm_stream stream);
/* Several slab reductions in ONE launch (small batches: a backward segment's weight-gradient GEMMs each leave a few small
 * slabs, and a launch per reduction costs more than the reduction).  `table` is a DEVICE array of `count` entries; every entry
 * keeps its own slab region until the call.  chunk0 = number of 256-float chunks of the entries before it (exclusive prefix sum of
 * ceil(n / 256)); `total_chunks` = that sum over all entries.  Deterministic slab order, like mmfm_reduce_slabs. */
typedef struct {
    float* dst;
    const float* src;
    int64_t n, slab_stride;
    int32_t nslabs, accumulate, chunk0, pad_;
} mmfm_reduce_entry;
int mmfm_reduce_slabs_multi(const mmfm_reduce_entry* table, int count, int total_chunks, mmfm_stream stream);
/* out[n] (+)= sum_r x[r*ld + n]   (bias gradients).  workspace >= mmfm_colsum_workspace bytes. */
int64_t mmfm_colsum_workspace(int64_t R, int N);
int mmfm_colsum(int dtype, const void* x, int64_t R, int N, int ld, float* out, int accumulate,
                void* workspace, int64_t workspace_bytes, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- LayerNorm
 * nn.LayerNorm(H), eps 1e-5, affine: encoder_embeddings.py:98,100; decoder_embeddings.py:118-126;
 * mm.py:72,77.  One wavefront per row, fp32 statistics.
 * destitch_T > 0: output row for input row r=(b,l) is (l/T)*(B*T) + b*T + l%T, i.e. the final
 * decoder_norm writes per-modality contiguous [M][B*T][H] blocks (the boolean gather of
 * decoder_embeddings.py:105 becomes a plain slice); the backward reads dy the same way. */
int mmfm_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y,
                       float* mean, float* rstd, int64_t R, int H, float eps,
                       int destitch_L, int destitch_T, mmfm_stream stream);
int64_t mmfm_layernorm_bwd_workspace(int64_t R, int H);
/* dx = dres + LN'(dy);  dgamma/dbeta (+)= column sums.  dres may be NULL; dx may alias dres. */
int mmfm_layernorm_bwd(int dtype, const void* dy, const void* x, const float* mean, const float* rstd,
                       const float* gamma, const void* dres, void* dx, float* dgamma, float* dbeta,
                       int accumulate, int64_t R, int H, int destitch_L, int destitch_T,
                       void* workspace, int64_t workspace_bytes, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- ScaleNorm
 * ScaleNorm(sqrt(H)) of `use_scalenorm: true` (mm_utils.py:31-39; encoder_embeddings.py:98,100; decoder_embeddings.py:118-126):
 *   y = x * g / max(||x||_2, eps)   per row, g ONE fp32 scalar (device pointer), fp32 statistics, one wavefront per row.
 * rinv[r] = 1 / max(||x_r||, eps), NEGATED for a clamped row (||x_r|| <= eps).  The backward (x_hat = x * |rinv|, v = g * dy):
 *   dx = dres + |rinv| * (v - x_hat * (x_hat . v))     (dx = dres + |rinv| * v for a clamped row: the clamp passes no gradient)
 *   dg (+)= sum over rows of x_hat . dy     (per-block partials in the workspace, reduced in a fixed order: deterministic)
 * dres may be NULL; dx may alias dres. */
int mmfm_scalenorm_fwd(int dtype, const void* x, const float* g, void* y, float* rinv, int64_t R, int H, float eps,
                       mmfm_stream stream);
int64_t mmfm_scalenorm_bwd_workspace(int64_t R, int H);
int mmfm_scalenorm_bwd(int dtype, const void* dy, const void* x, const float* rinv, const float* g, const void* dres, void* dx,
                       float* dg, int accumulate, int64_t R, int H, void* workspace, int64_t workspace_bytes,
                       mmfm_stream stream);

/* ---------------------------------------------------------------------------------- attention
 * F.scaled_dot_product_attention with the reference's masks (mm_utils.py:105-111,143-149;
 * mm.py:152-158,178-194) without materialising [B,h,L,L]:
 *   allowed(b,q,k) = (DIAG && q==k) | (CAUSAL ? k<=q : keypad[b][k]) | (SEP && mod_id[q]!=mod_id[k])
 * q/k/v/o are [B, L, heads*dh] views with row strides ldq/ldk/ldv/ldo (so a fused QKV buffer
 * works); lse is [B, heads, Lq] fp32.  drop_p acts on the probabilities, drop_o on the output
 * (the nn.Dropout in front of out_proj, mm_utils.py:114).
 * dh (the head dim, hidden_size / n_heads) is 8, 16, 32, 64 or 128; every other value is an error at launch, and
 * EngineConfig.from_model_config refuses it when the config is read.  Everything below holds at every one of them.  Which kernels
 * serve which dh: fp32 - csrc/attention.hip at all five; bf16 - the general MFMA kernels of csrc/attention_bf16.hip at 16, 32, 64
 * and 128 (at 128 always their chunk-streaming pair), fp32 compute on bf16 storage at 8; with the keep-bit workspace (keepbits
 * below) the fast kernels of csrc/attention_fast.hip at dh 32 and the kernels of csrc/attention_long.hip at dh 64 and 128.  Not
 * built: dh 128 on the dh-32 fast kernels' straight-line path (a head's K / V held in LDS for the whole launch), and any head dim
 * outside {8, 16, 32, 64, 128}. */
#define MMFM_ATTN_DIAG 1
#define MMFM_ATTN_CAUSAL 2
#define MMFM_ATTN_SEP 4
typedef struct {
    int dtype;
    int B, heads, Lq, Lk, dh;
    const void* q; const void* k; const void* v;
    int ldq, ldk, ldv;
    void* o; int ldo;            /* fwd: output (after drop_o).  bwd: the forward's output */
    float* lse;
    const uint8_t* keypad;       /* [B][Lk] */
    const uint8_t* mod_id;       /* [max(Lq,Lk)] or NULL */
    int flags;
    float scale;
    mmfm_dropout drop_p, drop_o;
    /* backward only */
    const void* d_o; int lddo;   /* grad wrt the out_proj input (i.e. AFTER drop_o) */
    void* dq; void* dk; void* dv;
    int lddq, lddk, lddv;
    /* optional (round 4): workspace of mmfm_attn_keepbits_bytes(B, heads, Lq, Lk) bytes for the keep decisions of drop_p, one bit
     * per (b, head, query, key).  With it, launches the dh = 32 fast kernels take (bf16, Lq <= 256, Lk <= 224, both % 8 == 0,
     * 16-B aligned operands; any combination of DIAG, CAUSAL and SEP) draw the decisions ONCE - mmfm_attn_fwd runs a generator
     * kernel in front of the forward - and mmfm_attn_bwd reads the same bits: the caller leaves the buffer alone between the two
     * calls.  Bits of elements the mask rule does not allow are unspecified (under CAUSAL / SEP whole tiles are never read).  The drop
     * probability is then honoured to 2^-10: keep = mmfm_attn_keep_prob(drop_p.p), survivors are scaled by 1 / keep.
     * NULL (or a shape the fast kernels do not take): both directions re-derive the decisions from the counter hash.
     * dh = 64 and dh = 128 (bf16, any Lq / Lk % 8 == 0, 16-B aligned operands, leading dims % 8 == 0; any combination of DIAG, CAUSAL and SEP,
     * CAUSAL / SEP with Lq == Lk): here the workspace SELECTS the kernel pair, with or without drop_p - a non-NULL keepbits sends
     * both directions to the keep-bit kernels, NULL to the general ones.  On that pair (i) dq is scratch until mmfm_attn_bwd
     * returns: a first kernel writes the output-dropout'd d_o there and the dQ phase overwrites it with dq, so dq must not alias
     * d_o, q, k or v; (ii) the tail of the workspace, behind the bit tiles, holds one float per (b, head, query) - the backward's
     * delta - which is why mmfm_attn_keepbits_bytes is more than the tiles; (iii) gradient tensors that are not 16-B aligned with
     * leading dims % 8 == 0 are an error, not a fallback (the forward already took its decisions from the bits).  The kernels'
     * LDS grows with Lk (key bias; under CAUSAL / SEP also a second bias row, the mod_id bytes and the tile votes): when the
     * forward or the dQ phase would need more than the 160 KB a workgroup can have (dh 64: Lk above ~22,000 dense, ~9,800 with CAUSAL /
     * SEP; dh 128, whose chunk images and transpose tiles take 136 KB: ~6,100 and ~2,600), the shape runs on the general kernels in
     * both directions, as every other shape this pair does not take.  The workspace layout and mmfm_attn_keepbits_bytes do not
     * depend on dh. */
    void* keepbits;
} mmfm_attn_desc;
int mmfm_attn_fwd(const mmfm_attn_desc* d, mmfm_stream stream);
int mmfm_attn_bwd(const mmfm_attn_desc* d, mmfm_stream stream);
int64_t mmfm_attn_keepbits_bytes(int B, int heads, int Lq, int Lk);
/* the keep probability the keep-bit path applies for a drop probability p */
float mmfm_attn_keep_prob(float p);
/* Which kernel family mmfm_attn_fwd (backward == 0) or mmfm_attn_bwd (backward != 0) runs for *d: one of the codes below, or a negative
 * code with mmfm_last_error set where the launch would refuse.  It launches nothing, reads no tensor (pointers count by being NULL or
 * not and by their alignment) and makes no HIP call: a machine without a GPU answers it.  A forward and its backward always name the
 * same family - the families draw the drop_p decisions from different sources - unless the gradient tensors alone keep the backward
 * off the bf16 kernels (not 16-B aligned, or leading dims % 8 != 0): then it is an error where drop_p is on or the family cannot be
 * left (KEEPBIT_LONG, BF16_TILED), and the next family down the list otherwise.  A backward on MMFM_ATTN_FAMILY_BF16 that runs the
 * single-pass kernel instead of the two-phase pair has MMFM_ATTN_FAMILY_BWD_SINGLE or-ed in.
 * MMFM_ATTN_FAMILY_MASK is the feature macro for this export (MMFM_VERSION stays, as for MMFM_NULL_BIAS: no existing struct changed). */
#define MMFM_ATTN_FAMILY_KEEPBIT_DH32 1   /* csrc/attention_fast.hip: bf16, dh 32, keep-bit workspace */
#define MMFM_ATTN_FAMILY_KEEPBIT_LONG 2   /* csrc/attention_long.hip: bf16, dh 64 / 128, keep-bit workspace */
#define MMFM_ATTN_FAMILY_BF16 3           /* csrc/attention_bf16.hip: bf16 MFMA, the head's images resident in LDS */
#define MMFM_ATTN_FAMILY_BF16_TILED 4     /* csrc/attention_bf16.hip: bf16 MFMA, chunk-streaming pair */
#define MMFM_ATTN_FAMILY_F32 5            /* csrc/attention.hip: fp32 compute (fp32 or bf16 storage), LDS-resident */
#define MMFM_ATTN_FAMILY_F32_TILED 6      /* csrc/attention.hip: fp32 compute, chunk-streaming pair */
#define MMFM_ATTN_FAMILY_MASK 0xf
#define MMFM_ATTN_FAMILY_BWD_SINGLE 0x10
int mmfm_attn_family(const mmfm_attn_desc* d, int backward);

/* MMFM_ATTN_WINDOW: attention inside a window over TIME STAMPS (mm.yaml context.forward / context.backward; upstream's
 * create_context_mask, mm_utils.py:18-34, which its forward_mask_encoder leaves commented out at mm.py:152-158).  pos[b][i] is the
 * time stamp of token i of sample b - not its index in the stitched sequence - and the rule of the window calls is
 *   allowed(b,q,k) = (DIAG && q==k) | (keypad[b][k] && lo <= pos[b][k] - pos[b][q] <= hi).
 * (lo, hi) for a config (F, Bk) = (context.forward, context.backward): hi = F >= 0 ? F : 2^30, lo = Bk > 0 ? -Bk : -2^30 (upstream's
 * `if context_backward > 0`: backward 0 is unbounded, like -1).  lo / hi beyond +-2^30 are clamped to it; mmfm_attn_pos_prep clamps the
 * stamps to +-2^29, so a difference always fits beside them.
 * The descriptor is mmfm_attn_desc as it is (MMFM_VERSION stays).  win == NULL is mmfm_attn_fwd / _bwd, the same launch.  Refused with
 * an error code and mmfm_last_error set, before any HIP call: Lq != Lk, CAUSAL or SEP in flags (not built under a window; no site of
 * the model needs them), pos == NULL.  Kernels: the general families - csrc/attention.hip (F32, F32_TILED) and
 * csrc/attention_bf16.hip (BF16, BF16_TILED), which stage the sample's pos row in LDS (4 bytes per position on top of their LDS
 * formulas) and never take their mask-free shortcut under a window - and the keep-bit dh-32 kernels (csrc/attention_fast.hip), whose
 * window forms classify (query tile, key tile) pairs from per-tile stamp minima / maxima: a launch they take (the shapes of keepbits
 * above) stays on them, keep bits and all.  csrc/attention_long.hip (dh 64 / 128 keep-bit) has no window form: such a launch runs
 * BF16 / BF16_TILED in both directions and draws drop_p from the counter hash even with a keepbits workspace; mmfm_attn_win_family
 * says which.  A query row with no allowed key gives NaN, as in mmfm_attn_fwd. */
#define MMFM_ATTN_WINDOW 1
typedef struct { const int32_t* pos; /* [B][L], L = Lq = Lk */ int lo, hi; } mmfm_attn_window;
int mmfm_attn_win_fwd(const mmfm_attn_desc* d, const mmfm_attn_window* win, mmfm_stream stream);
int mmfm_attn_win_bwd(const mmfm_attn_desc* d, const mmfm_attn_window* win, mmfm_stream stream);
/* no HIP call, as mmfm_attn_family */
int mmfm_attn_win_family(const mmfm_attn_desc* d, const mmfm_attn_window* win, int backward);
/* pos[b][off_j + t] = clamp(ts[j][b * seg_T[j] + t], -2^29, 2^29) for the M slots of a stitched sequence (off_j = sum_{i<j} seg_T[i],
 * L = sum seg_T; the uniform form passes the one shared stamp tensor M times).  seg_T and ts are HOST arrays read during the call (they
 * travel as launch arguments: no allocation, hipGraph-capturable); M <= MMFM_MAX_SEGMENTS.  Arguments are checked before any HIP call. */
int mmfm_attn_pos_prep(int B, int M, const int32_t* seg_T, const int64_t* const* ts, int32_t* pos, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- masks / stitch
 * mm.py:245-275 (mask = eval_mask[:,:,0] & attn_mask), :102 (mod_mask), :145,167 (sample-0 ids),
 * :229-233 (n_examples).  For modality m: mask_src[m] is int64 with element (b,t) at
 * mask_src[m][(b*T+t)*mask_stride[m]]; attn is int64 [B][T].
 * Outputs: tokmask u8 [B][M*T], keypad u8 [B][M*T], keep0 u8 [M*T] (0 where sample 0 is masked),
 * mod_id u8 [M*T], count int64 [M] = channels[m] * sum(tokmask of modality m).  Bit-exact. */
int mmfm_mask_prep(int B, int T, int M, const int64_t* const* mask_src, const int64_t* mask_stride,
                   const int64_t* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad,
                   uint8_t* keep0, uint8_t* mod_id, int64_t* count, mmfm_stream stream);

/* encoder_embeddings.py:56-61 + mm.py:90-110,143-149,289 (and the decoder twins):
 *   emb[b, m*T+t] = mod_emb[mod_row] + pos_emb[ts[b][t]]
 *   x  [b, m*T+t] = keep0[m*T+t] * tok[b*T+t] + emb[...]
 * called once per modality m; tok is [B*T][H]; x/emb are [B][L][H]; emb may be NULL; pos_emb has
 * max_F rows (time stamps are clamped into [0, max_F) for memory safety).
 * pos_emb == NULL (embedder.pos: false, MMFM_EMBED_OPTS): emb = mod_emb[mod_row], the same row for every token; ts may be passed and
 * is not read (it may be NULL too). */
int mmfm_stitch_fwd(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb,
                    const int64_t* ts, const uint8_t* keep0, void* x, void* emb,
                    int B, int T, int L, int m, int H, int max_F, mmfm_stream stream);
/* autograd of the above for one modality: d_tok[b*T+t] = keep0 * dropout'(dx[b, m*T+t]);
 * d_mod_row (+)= sum_{b,t} (dx + dextra);  d_pos[ts[b][t]] (+)= dx + dextra  (dextra may be NULL:
 * it is d_context -> encoder_emb, mm.py:292).  acc_mod / acc_pos select += for each output (the
 * modality embedding is shared by the encoder and decoder tokenisers, mm.py:84-87, the position
 * tables are not).  Deterministic (no atomics): fp32 mode scatters through per-column LDS tables and reduces the
 * per-chunk partials; bf16 mode (H % 8 == 0) multiplies by a one-hot matrix on the MFMA GEMM ([d_pos; d_mod] = OH^T E,
 * split-K slabs, fixed-order reduction).
 * d_pos == NULL (embedder.pos: false, MMFM_EMBED_OPTS): d_tok and d_mod_row only; ts is not read, acc_pos is ignored.  fp32 mode runs without
 * the LDS tables; in bf16 mode the one-hot product degenerates to a column sum over the modality's rows (per-sample-range slabs, summed in
 * a fixed order: deterministic, no atomics).  Both stay within mmfm_stitch_bwd_workspace(...), which is the same for either form. */
int64_t mmfm_stitch_bwd_workspace(int dtype, int B, int T, int L, int H, int max_F);
int mmfm_stitch_bwd(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0,
                    mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos,
                    int B, int T, int L, int m, int H, int max_F,
                    void* workspace, int64_t workspace_bytes, mmfm_stream stream);
/* The same with tok / d_tok over the compact row space of the slot's live-bin record `rec` (mmfm_live_bins; keep0 is the one it was made
 * from): the forward reads tok at row b * T_live + rank[t], the backward writes d_tok for live rows only, at their compact rows (the
 * dropout counter stays the original row's).  Everything else - emb, d_mod_row, d_pos - covers all rows as above. */
int mmfm_stitch_fwd_live(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb,
                         const int64_t* ts, const uint8_t* keep0, const int32_t* rec, void* x, void* emb,
                         int B, int T, int L, int m, int H, int max_F, mmfm_stream stream);
int mmfm_stitch_bwd_live(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0, const int32_t* rec,
                         mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos,
                         int B, int T, int L, int m, int H, int max_F,
                         void* workspace, int64_t workspace_bytes, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- modality segments
 * MMFM_MOD_SEGMENTS: the edges of the model over modalities of different length.  Upstream concatenates along the token axis
 * (mm.py:97-138), every tokeniser looks up its own time stamps (encoder_embeddings.py:56-59), the key mask is the concatenation of the
 * per-modality masks (mm.py:152-158) and the heads pick their rows with y[decoder_mod_mask == mod_idx] (decoder_embeddings.py:105-107).
 * Slot j of a side's stitched sequence has its own length T_j, time stamps ts_j [B][T_j] and attention mask attn_j [B][T_j]; it starts
 * at off_j = sum_{i<j} T_i and L = sum_j T_j.  The entry points above are the case T_j = T, ts_j = ts, attn_j = attn, off_j = j * T,
 * and at that case these give the same bits.  At most MMFM_MAX_SEGMENTS slots; seg_T is a HOST array read during the call (the table
 * travels to the kernels as launch arguments: no allocation, hipGraph-capturable).  Everything between the edges - attention, the
 * row-owner linears, the MLP, the weight gradients, the masked loss (base pointer, mask_ld = L, T = T_j) - takes R = B * L rows as it is.
 * The live-bin entry points (mmfm_live_bins, the _live stitches, mmfm_gather_live_rows) have no segment forms. */
#define MMFM_MOD_SEGMENTS 1
#define MMFM_MAX_SEGMENTS 8
/* mmfm_mask_prep over segments: mask_src[j] has element (b,t) at mask_src[j][(b*seg_T[j]+t)*mask_stride[j]], attn[j] is int64
 * [B][seg_T[j]] (mask_src and attn are host arrays of M device pointers).  Outputs as mmfm_mask_prep with M*T replaced by L:
 * tokmask, keypad u8 [B][L], keep0, mod_id u8 [L] (mod_id = the slot j), count int64 [M] = channels[j] * sum(tokmask of slot j).
 * Bit-exact. */
int mmfm_mask_prep_seg(int B, int M, const int32_t* seg_T, const int64_t* const* mask_src, const int64_t* mask_stride,
                       const int64_t* const* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad,
                       uint8_t* keep0, uint8_t* mod_id, int64_t* count, mmfm_stream stream);
/* mmfm_stitch_fwd / _bwd for the slot of T bins at offset off (off + T <= L) - the same kernels at another offset: the uniform entry
 * points are these at off = m * T:
 *   emb[b, off+t] = mod_emb[mod_row] + pos_emb[ts[b][t]],   x[b, off+t] = keep0[off+t] * tok[b*T+t] + emb[...]
 *   d_tok[b*T+t] = keep0[off+t] * dropout'(dx[b, off+t]);  d_mod_row (+)= sum_{b,t} (dx + dextra);  d_pos[ts[b][t]] (+)= dx + dextra
 * tok / d_tok are [B*T][H], ts is the slot's own [B][T].  The NULL pos_emb / d_pos contract (MMFM_EMBED_OPTS), acc_mod / acc_pos, the
 * dropout counter (the row b*T+t inside the modality, times H, plus the column) and the determinism (no atomics, fixed-order
 * reductions; bf16 with H % 8 == 0: the one-hot product, or its column sum without a table) are those of mmfm_stitch_fwd / _bwd. */
int mmfm_stitch_fwd_seg(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb,
                        const int64_t* ts, const uint8_t* keep0, void* x, void* emb,
                        int B, int T, int L, int off, int H, int max_F, mmfm_stream stream);
int64_t mmfm_stitch_bwd_seg_workspace(int dtype, int B, int T, int L, int off, int H, int max_F);
int mmfm_stitch_bwd_seg(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0,
                        mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos,
                        int B, int T, int L, int off, int H, int max_F,
                        void* workspace, int64_t workspace_bytes, mmfm_stream stream);
/* ---------------------------------------------------------------------------------- per-sample token masks
 * MMFM_TOKEN_MASK_ROWS: x[b, l] = keep[b][l] * tok[b, l] + emb[b, l] with every sample's own keep row,
 * keep[b][l] = (v[b][l] != 1), v = mask & attn - upstream's comparison (mm.py:145 `mask[0] == 1`) applied per sample, so at B = 1
 * it is the keep0 of the entry points above.  What `tokens[mask == 1] = 0` would do; MultiModal.per_sample_mask.
 *
 * mmfm_mask_prep_rows takes the argument list of mmfm_mask_prep_seg (the uniform form passes seg_T[j] = T and one attention mask M
 * times).  tokmask, keypad, mod_id and count are those of mmfm_mask_prep / _seg, bit for bit; keep is u8 [B][L]; keep_any u8 [L] is
 * keep_any[l] = OR_b keep[b][l] - the mask to make live-bin records from (mmfm_live_bins): a bin is dead only where every sample
 * masks it.  Integers only, deterministic, no allocation, hipGraph-capturable. */
#define MMFM_TOKEN_MASK_ROWS 1
int mmfm_mask_prep_rows(int B, int M, const int32_t* seg_T, const int64_t* const* mask_src, const int64_t* mask_stride,
                        const int64_t* const* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad,
                        uint8_t* keep, uint8_t* keep_any, uint8_t* mod_id, int64_t* count, mmfm_stream stream);
/* One stitch pair for the slot of T bins at offset off with the slot's own ts [B][T] - what the uniform, _seg and _live entry points
 * cover - under a keep mask given as base pointer and row stride: element (b, off + t) at keep[b * keep_ld + off + t].  keep_ld = 0 is
 * the one shared row of the entry points above, and then these give the bits of mmfm_stitch_*_seg (rec == NULL) and of
 * mmfm_stitch_*_live (rec given, off = m * T); keep_ld >= L is a per-sample mask (mmfm_mask_prep_rows: keep_ld = L).
 * rec: NULL, or the slot's live-bin record made from keep_any (bf16 only): tok / d_tok are then over the compact rows.  Under a
 * per-sample mask a live bin can be masked in some samples: the forward does not read that compact tok row, and the backward writes
 * ZEROS to that compact d_tok row (the weight-gradient product over the compact rows reads it); rows of dead bins do not exist.
 * The NULL pos_emb / d_pos contract (MMFM_EMBED_OPTS), acc_mod / acc_pos, the dropout counter (the original row b*T+t, times H, plus
 * the column), the workspace (mmfm_stitch_bwd_seg_workspace) and the determinism are those of the entry points above.
 * Argument errors return before any HIP call: keep_ld neither 0 nor >= L, off + T > L, rec given in fp32. */
int mmfm_stitch_fwd_rows(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb,
                         const int64_t* ts, const uint8_t* keep, int keep_ld, const int32_t* rec, void* x, void* emb,
                         int B, int T, int L, int off, int H, int max_F, mmfm_stream stream);
int mmfm_stitch_bwd_rows(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep, int keep_ld,
                         const int32_t* rec, mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos,
                         int B, int T, int L, int off, int H, int max_F,
                         void* workspace, int64_t workspace_bytes, mmfm_stream stream);
/* mmfm_layernorm_fwd / _bwd de-stitching over segments: with B = R / L, the output row for input row r = (b, off_j + t) is
 * B*off_j + b*seg_T[j] + t, so the final decoder_norm writes one contiguous [B*T_j][H] block per decoder modality, slot j's at row
 * B*off_j; the backward reads dy the same way.  Workspace: mmfm_layernorm_bwd_workspace(R, H). */
int mmfm_layernorm_fwd_seg(int dtype, const void* x, const float* gamma, const float* beta, void* y,
                           float* mean, float* rstd, int64_t R, int H, float eps,
                           int n_seg, const int32_t* seg_T, mmfm_stream stream);
int mmfm_layernorm_bwd_seg(int dtype, const void* dy, const void* x, const float* mean, const float* rstd,
                           const float* gamma, const void* dres, void* dx, float* dgamma, float* dbeta,
                           int accumulate, int64_t R, int H, int n_seg, const int32_t* seg_T,
                           void* workspace, int64_t workspace_bytes, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- loader collate
 * BaseDataset._preprocess_ibl_data + get_binned_spikes_from_sparse (loader/base.py:304-450,
 * utils/dataset_utils.py:38-43), pad_to_right path: B trials given as concatenated CSR pieces
 * (uint8 counts, int32 column indices, int64 row pointers) -> dense spikes [B][max_T][max_N] fp32,
 * rows/columns beyond a trial's (T_b, N_b) = pad_value, longer trials truncated; time_mask [B][max_T]
 * and space_mask [B][max_N] int64 (1 = real data).  Duplicate (row, col) entries add up. */
int mmfm_collate_csr(int B, int max_T, int max_N, float pad_value, const uint8_t* data, const int32_t* indices,
                     const int64_t* indptr, const int64_t* indptr_off, const int64_t* nnz_off, const int32_t* T_b,
                     const int32_t* N_b, float* out, int64_t* time_mask, int64_t* space_mask, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- masked loss
 * mm.py:79-82,217-239: an elementwise loss of (pred, target), times the [B,T] token mask, summed.  With d = p - t and
 * `param` the kind's one float (ignored by the kinds that have none; must be >= 0):
 *   kind                          torch module (reduction="none")          element                                  d/dp
 *   0 MMFM_LOSS_POISSON_LOG       PoissonNLLLoss(log_input=True)           exp(p) - t p                             exp(p) - t
 *   1 MMFM_LOSS_MSE               MSELoss                                  d^2                                      2 d
 *   2 MMFM_LOSS_POISSON_RATE      PoissonNLLLoss(log_input=False, eps)     p - t log(p + eps)                       1 - t / (p + eps)
 *   3 MMFM_LOSS_L1                L1Loss                                   |d|                                      sign(d), 0 at d == 0
 *   4 MMFM_LOSS_SMOOTH_L1         SmoothL1Loss(beta)                       |d| < beta ? d^2 / (2 beta) : |d| - beta/2     |d| < beta ? d / beta : sign(d)
 *   5 MMFM_LOSS_HUBER             HuberLoss(delta)                         |d| <= delta ? d^2 / 2 : delta (|d| - delta/2) |d| <= delta ? d : delta sign(d)
 *   6 MMFM_LOSS_BCE_LOGITS        BCEWithLogitsLoss()                      max(p,0) - p t + log1p(exp(-|p|))        sigmoid(p) - t
 * beta == 0 makes kind 4 the L1 loss, as in torch.  flags: MMFM_LOSS_FULL (kinds 0 and 2 only) = PoissonNLLLoss(full=True): adds
 * Stirling's t log t - t + log(2 pi t) / 2 to the elements with t > 1; it has no gradient.
 * pred [R][N] (dtype), target [R][N] fp32, rowmask u8 [R] (element (b,t) at rowmask[b*mask_ld + t]).
 * fwd writes the modality's masked SUM to loss_sum[0] (fp32, deterministic two-stage).
 * mmfm_masked_loss_fwd / _bwd are the two-kind entry points of every earlier 401 library (kind 0 or 1, no parameter, no flag) and
 * stay as they were; mmfm_masked_loss_kind_fwd / _bwd take every kind, 0 and 1 included (same kernels, same bits), and share
 * mmfm_masked_loss_workspace.  MMFM_LOSS_KINDS is the feature macro for them (MMFM_VERSION stays, as for MMFM_NULL_BIAS). */
#define MMFM_LOSS_KINDS 1
#define MMFM_LOSS_POISSON_LOG 0
#define MMFM_LOSS_MSE 1
#define MMFM_LOSS_POISSON_RATE 2
#define MMFM_LOSS_L1 3
#define MMFM_LOSS_SMOOTH_L1 4
#define MMFM_LOSS_HUBER 5
#define MMFM_LOSS_BCE_LOGITS 6
#define MMFM_LOSS_FULL 1
int64_t mmfm_masked_loss_workspace(int64_t R, int N);
int mmfm_masked_loss_fwd(int dtype, int kind, const void* pred, const float* target, const uint8_t* rowmask,
                         int mask_ld, int T, int64_t R, int N, float* loss_sum,
                         void* workspace, int64_t workspace_bytes, mmfm_stream stream);
int mmfm_masked_loss_kind_fwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                              const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, float* loss_sum,
                              void* workspace, int64_t workspace_bytes, mmfm_stream stream);
/* loss = sum_m loss_sum[m] / sum_m count[m]   (0/0 -> NaN like the reference);  inv_n = 1/sum count */
int mmfm_loss_finalize(const float* loss_sum, const int64_t* count, int M, float* loss, float* inv_n,
                       mmfm_stream stream);
/* dpred = grad_out[0] * inv_n[0] * rowmask * d/dp loss_elem: exactly 0 on un-masked rows, NaN everywhere when inv_n is inf
 * (nothing masked in any modality) */
int mmfm_masked_loss_bwd(int dtype, int kind, const void* pred, const float* target, const uint8_t* rowmask,
                         int mask_ld, int T, int64_t R, int N, const float* grad_out, const float* inv_n,
                         void* dpred, mmfm_stream stream);
int mmfm_masked_loss_kind_bwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                              const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const float* grad_out,
                              const float* inv_n, void* dpred, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- masked loss under a per-element mask
 * Input masking (mask_type: input): the loss mask is per element, logically u8 [B][T][N], and is passed in whatever compact form the
 * caller holds - a base pointer and three element strides, any of which may be 0: element (b,t,n) sits at
 * mask[b*sb + t*st + n*sn].  A [B,1,N] tensor is (N, 0, 1), a [1,T,1] tensor (0, 1, 0), a full contiguous one (T*N, N, 1); nothing
 * is expanded in memory.  pred [B*T][N] (dtype), target [B*T][N] fp32, every kind and flag of mmfm_masked_loss_kind_*.
 *   fwd  loss_sum[0] = sum of the elements whose mask is set (fixed-order two-stage sum), count[0] = their exact number (int64; per-block
 *        integer partials, summed by the second stage).  No memset, no floating-point atomic, the same bits on every call.  An element
 *        whose mask is 0 is never loaded: a NaN or Inf there does not reach the sum.
 *   bwd  dpred = grad_out[0] * inv_n[0] * d/dp on set elements, that factor times 0 on the others (exactly 0, or NaN when inv_n is inf).
 * Rows, lanes and columns are walked as mmfm_masked_loss_kind_* walk them: an all-ones mask gives their bits with every row masked, a
 * [B,T,1] mask their bits with that row mask.  workspace: mmfm_masked_loss_elem_workspace bytes, 8-byte aligned.
 *
 * mmfm_stage_masked: dst[b,t,n] = cm(b,t,n) ? 0 : src[b,t,n] for n < N - the staging copy of a batch's inputs with the masker's
 * zeroing folded in.  src fp32 [B*T][N] contiguous, cm a strided mask as above, dst [B*T][ld_dst] of `dtype` (ld_dst >= N; columns
 * N.. are not written).  16-byte accesses where N, ld_dst and the two base pointers allow.
 *
 * Argument checks (null pointers, dtype, kind / param / flags, sizes, negative strides, workspace) return -1 before any HIP call; no
 * call allocates or synchronises.  MMFM_LOSS_ELEM is the feature macro for the four exports (MMFM_VERSION stays, as for MMFM_LOSS_KINDS). */
#define MMFM_LOSS_ELEM 1
int64_t mmfm_masked_loss_elem_workspace(int64_t R, int N);
int mmfm_masked_loss_elem_fwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                              const uint8_t* mask, int64_t sb, int64_t st, int64_t sn, int B, int T, int N, float* loss_sum,
                              int64_t* count, void* workspace, int64_t workspace_bytes, mmfm_stream stream);
int mmfm_masked_loss_elem_bwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                              const uint8_t* mask, int64_t sb, int64_t st, int64_t sn, int B, int T, int N,
                              const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream);
int mmfm_stage_masked(int dtype, const float* src, const uint8_t* cm, int64_t sb, int64_t st, int64_t sn, int B, int T, int N,
                      void* dst, int ld_dst, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- masked loss under a row mask x channel mask
 * Padded neurons (space_attn_mask): the loss mask is the product of the [B,T] token mask and a [B,N] channel mask, kept as the two
 * factors.  Element (row, c) with b = row / T, t = row % T is set iff rowmask[b*mask_ld + t] && chanmask[b*chan_ld + c]; mask_ld == 0
 * is one row mask u8 [T] for all samples, chan_ld == 0 one channel mask u8 [N] for all samples (otherwise mask_ld >= T, chan_ld >= N).
 * pred [R][N] (dtype), target [R][N] fp32, every kind and flag of mmfm_masked_loss_kind_* (kind 7 is "bad kind" here too).
 *   fwd  loss_sum[0] = sum over the set elements (fixed-order two-stage sum), count[0] = their exact number (int64, integer partials).
 *        A row whose rowmask is 0 is skipped without loading any of its pred / target; in a masked row an element whose channel bit is
 *        0 is never loaded; a sample's channel-mask bytes are read once per masked row.  No memset, no floating-point atomic, no
 *        allocation, no synchronisation; the same bits on every call.
 *   bwd  writes every element of dpred: grad_out[0] * inv_n[0] * d/dp on set elements, that factor times 0 on the others (exactly 0, or
 *        NaN when inv_n is inf).
 * Rows, lanes and columns are walked as mmfm_masked_loss_kind_* walk them: an all-ones channel mask gives their bits (and count =
 * masked rows x N), any mask pair the bits of mmfm_masked_loss_elem_* on the expanded [B,T,N] product.  workspace:
 * mmfm_masked_loss_chan_workspace bytes, 8-byte aligned.  Argument checks (null pointers, dtype, kind / param / flags, sizes, negative
 * leading dimensions, R % T != 0, workspace) return -1 before any HIP call.  MMFM_LOSS_CHAN is the feature macro for the three exports
 * (MMFM_VERSION stays, as for MMFM_LOSS_KINDS). */
#define MMFM_LOSS_CHAN 1
int64_t mmfm_masked_loss_chan_workspace(int64_t R, int N);
int mmfm_masked_loss_chan_fwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                              const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const uint8_t* chanmask, int chan_ld,
                              float* loss_sum, int64_t* count, void* workspace, int64_t workspace_bytes, mmfm_stream stream);
int mmfm_masked_loss_chan_bwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                              const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const uint8_t* chanmask, int chan_ld,
                              const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- softmax cross-entropy (categorical modalities)
 * Kind 7, the one loss whose row elements are coupled (a log-sum-exp over the N classes of a row), with entry points of its own:
 * mmfm_masked_loss_kind_fwd / _bwd answer "bad kind" for it.  For logits p[c], targets t[c] (one-hot or any non-negative weights, not
 * necessarily summing to 1), class weights w[c] (class_weight == NULL: 1) and label smoothing eps in [0, 1]:
 *   t'[c]   = (1 - eps) t[c] + eps / N
 *   e[c]    = - w[c] t'[c] log_softmax(p)[c]                 the [R][N] tensor upstream multiplies by the token mask (mm.py:217-239)
 *   row     = sum_c e[c] = sum_c w[c] t'[c] (lse(p) - p[c])  = F.cross_entropy(p, t, weight=w, label_smoothing=eps, reduction='none')
 *   d/dp[j] = softmax(p)[j] sum_c w[c] t'[c] - w[j] t'[j]
 * and n_examples stays N * (masked rows), upstream's targets_mask.sum() over [B,T,N]: what mmfm_mask_prep counts with channels = N.
 * pred [R][N] (dtype), target [R][N] fp32, rowmask as above; un-masked rows are never read by the forward.  fp32 arithmetic, the row
 * maximum subtracted before the exponential; fwd writes the masked SUM to loss_sum[0] (fixed-order two-stage sum, the same bits on
 * every call; no allocation, no sync, no floating-point atomic).  A row is owned by G lanes, G the smallest power of two
 * >= min(N, 64), 64 / G rows to a wavefront; for N > 64 a wavefront owns the row and its lanes stride over the columns.
 * rowstat (or NULL) [R][2] fp32: fwd leaves (lse, sum_c w t') of every MASKED row there (other rows are not written); bwd reads them
 * when given - one pass over the row - and recomputes them otherwise, to the same bits.  bwd writes dpred as mmfm_masked_loss_bwd
 * does: grad_out[0] * inv_n[0] * d/dp on masked rows, that factor times 0 on the others (exactly 0, or NaN when inv_n is inf).
 * Non-finite logits are outside the contract.
 *
 * mmfm_argmax_confusion: conf[N][N] int64 is OVERWRITTEN with the counts of (arg-max of target, arg-max of pred) over the masked
 * rows (rowmask == NULL: every row), row = target class; the lowest index wins a tie in both.  Exact (integer atomics).
 *
 * Argument checks (null pointers, dtype, label_smoothing outside [0, 1], R % T != 0, mask_ld < T, workspace size) return -1 before
 * any HIP call.  MMFM_SOFTMAX_CE is the feature macro (MMFM_VERSION stays, as for MMFM_LOSS_KINDS). */
#define MMFM_SOFTMAX_CE 1
#define MMFM_LOSS_SOFTMAX_CE 7
int64_t mmfm_softmax_ce_workspace(int64_t R, int N);
int mmfm_softmax_ce_fwd(int dtype, const void* pred, const float* target, const float* class_weight /* [N] or NULL */,
                        float label_smoothing, const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N,
                        float* loss_sum, float* rowstat /* [R][2] = (lse, sum w t') of masked rows, or NULL */,
                        void* workspace, int64_t workspace_bytes, mmfm_stream stream);
int mmfm_softmax_ce_bwd(int dtype, const void* pred, const float* target, const float* class_weight, float label_smoothing,
                        const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const float* rowstat /* NULL: recompute */,
                        const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream);
int mmfm_argmax_confusion(int dtype, const void* pred, const float* target, const uint8_t* rowmask /* or NULL */, int mask_ld,
                          int T, int64_t R, int N, int64_t* conf /* [N][N], row = target class */, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- elementwise
 * dst = dropout(src) with counter row*N + col (the backward of a dropout whose forward was fused
 * into a GEMM epilogue). */
int mmfm_dropout_apply(int dtype, const void* src, void* dst, int64_t R, int N, mmfm_dropout drop,
                       mmfm_stream stream);
int mmfm_cast_f32_to_bf16(const float* src, void* dst, int64_t n, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- optimiser
 * torch.optim.AdamW single step over a flat fp32 parameter range (train_multi_modal.py:197-202,
 * trainer/base.py:196).  hyper is a DEVICE array of 8 floats the host computes in double:
 *   [1-lr*wd, 1-beta1, beta2, 1-beta2, lr/bias_correction1, sqrt(bias_correction2), eps, grad_scale]
 * (OneCycleLR rewrites lr AND beta1 every step, so they are data, not launch constants; g is
 * multiplied by grad_scale first, e.g. 1/world_size after a SUM all-reduce).
 * If p_bf16 != NULL the updated parameters are also written as bf16 (throughput mode weights). */
int mmfm_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                    const float* hyper, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- optimiser over a range table
 * Param groups, frozen parameters and gradient clipping: the same update over RANGES of the flat buffers, each with its own hyper row.
 * MMFM_OPTIM_RANGES is the feature macro for everything below (MMFM_VERSION stays, as for MMFM_NULL_BIAS: mmfm_adamw_step and every
 * existing struct are unchanged).
 *
 * A range is [start, end) in elements of p / g / m / v and names a row of hyper[hyper_rows][8] (the layout of mmfm_adamw_step's hyper).
 * Ranges are HOST memory, non-empty, sorted by start and disjoint; elements outside every range are never read or written.
 *
 * The host cuts the ranges at the multiples of MMFM_OPTIM_CHUNK elements (counted from element 0 of the buffer, so that a chunk never
 * straddles a 16 KiB window and its interior is 16-byte aligned whenever the buffers are): range r becomes the chunks
 *   [max(start, k * CHUNK), min(end, (k + 1) * CHUNK))   for k = start / CHUNK .. (end - 1) / CHUNK,
 * in range order.  mmfm_optim_ranges_chunks counts them, mmfm_optim_ranges_table writes the table into HOST memory:
 *   mmfm_optim_chunk chunk[n_chunks];  int32 first_chunk[n_ranges + 1]     (mmfm_optim_ranges_table_bytes in all)
 * which the caller copies to the device once per set of ranges (not per step) and passes as `table`.  A workgroup owns whole chunks and
 * reads range and hyper row from the table; which lane handles which element follows from the element's index alone, so neither grid
 * size nor occupancy changes any bit of the results.
 *
 * Argument checks (NULL pointers; empty, unsorted or overlapping ranges; a range past n; a hyper row outside [0, hyper_rows); an
 * n_chunks that is not the count of these ranges) return -1 before any HIP call: a machine without a GPU answers them. */
#define MMFM_OPTIM_RANGES 1
#define MMFM_OPTIM_CHUNK 4096
typedef struct {
    int64_t start, end;      /* [start, end) in elements */
    int32_t hyper_row;
    int32_t reserved;
} mmfm_optim_range;
typedef struct {
    int64_t start;           /* first element */
    int32_t len;             /* 1 .. MMFM_OPTIM_CHUNK, inside one CHUNK-aligned window */
    int32_t range;           /* index of the range it was cut from */
    int32_t hyper_row;
    int32_t reserved;
} mmfm_optim_chunk;
/* The device record mmfm_grad_sumsq_ranges leaves at the start of its workspace (workspace = record, double range_sumsq[n_ranges],
 * double chunk_partial[n_chunks]).  `skipped` is the only field a call reads before writing: zero the workspace once before first use. */
typedef struct {
    double total;            /* sum of range_sumsq, added in range order */
    float clip_coef;         /* min(1, max_norm / (sqrt(total) + 1e-6)), formed in double; 1 where max_norm <= 0, inf or NaN */
    int32_t nonfinite;       /* 1 where any chunk partial (or the total) is inf or NaN */
    int64_t skipped;         /* incremented by every call with skip_nonfinite != 0 that set nonfinite */
    int32_t n_ranges;
    int32_t reserved;
} mmfm_optim_record;
/* Number of chunks of these ranges (>= n_ranges), or -1 with mmfm_last_error set.  HOST only. */
int64_t mmfm_optim_ranges_chunks(const mmfm_optim_range* ranges, int n_ranges, int64_t n, int hyper_rows);
int64_t mmfm_optim_ranges_table_bytes(int64_t n_chunks, int n_ranges);
/* Writes the table described above into table_host[table_bytes].  HOST only. */
int mmfm_optim_ranges_table(const mmfm_optim_range* ranges, int n_ranges, int64_t n, int hyper_rows, void* table_host, int64_t table_bytes);
/* Bytes of record + per-range sums + per-chunk partials. */
int64_t mmfm_optim_ranges_workspace(int64_t n_chunks, int n_ranges);
/* range_sumsq[r] = sum over range r of x^2 with x = g * coef_in rounded to fp32 (what the update forms: pass coef_in = grad_scale), every
 * product and addition in fp64.  Two launches, no floating-point atomics: one partial per chunk (fixed lane assignment, fixed reduction
 * tree), then one workgroup adds each range's partials in chunk order, the range sums in range order, and writes the record.
 * Same inputs, same bits.  max_norm <= 0 or inf: no clipping (clip_coef = 1); a NaN total also gives clip_coef = 1. */
int mmfm_grad_sumsq_ranges(const float* g, int64_t n, const mmfm_optim_range* ranges, int n_ranges, const void* table, int64_t n_chunks,
                           float coef_in, float max_norm, int skip_nonfinite, void* workspace, int64_t workspace_bytes,
                           mmfm_stream stream);
/* mmfm_adamw_step's update over every chunk with the chunk's hyper row; the gradient is gi = (g * clip_coef) * grad_scale, in that
 * order, clip_coef read from *record (DEVICE; NULL: 1).  With skip_nonfinite != 0 and record->nonfinite set every workgroup returns
 * before its first store: p, m, v and p_bf16 keep every byte.  p_bf16 as in mmfm_adamw_step. */
int mmfm_adamw_step_ranges(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const mmfm_optim_range* ranges,
                           int n_ranges, const void* table, int64_t n_chunks, const float* hyper, int hyper_rows,
                           const mmfm_optim_record* record, int skip_nonfinite, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- gradient accumulation
 * torch's `p.grad += new` for a backward that OVERWRITES its gradient buffer: stash the range before the backward, add it back after.
 * MMFM_GRAD_ACCUM is the feature macro for this export (MMFM_VERSION stays, as for MMFM_NULL_BIAS: no existing struct changed).
 *
 * Both modes work over elements [start, end) of two flat fp32 buffers of n elements:
 *   MMFM_GRAD_STASH   stash[i] = g[i]
 *   MMFM_GRAD_ADD     g[i] = g[i] + stash[i]
 * 16-byte accesses over the interior that is 16-byte aligned in both buffers, element accesses over its head and tail (over the whole
 * range where the buffers disagree modulo 16 bytes).  Exactly one lane handles each element; no atomics, no reduction: neither grid
 * size nor occupancy changes any bit.  Elements outside the range are neither read nor written.  One launch, no allocation, no
 * synchronisation (capturable); start == end returns 0 without a launch.
 * Argument checks (NULL pointers, start < 0, end > n, start > end, an unknown mode) return -1 before any HIP call: a machine without a
 * GPU answers them. */
#define MMFM_GRAD_ACCUM 1
#define MMFM_GRAD_STASH 0
#define MMFM_GRAD_ADD 1
int mmfm_grad_accumulate(float* g, float* stash, int64_t n, int64_t start, int64_t end, int mode, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- per-session linear layers (use_session)
 * A per-session read-in from the session's n_s neurons to a shared width P and a read-out from P back to n_s, over a batch whose
 * samples may belong to different sessions.  MMFM_SESSION_LINEAR is the feature macro for these exports (MMFM_VERSION stays: no
 * existing struct or kernel changed).
 *
 * Every session fact is DEVICE data, so that a captured launch serves every session and every mix of sessions of one batch shape:
 *   sid[B]      the session of each sample
 *   n[S]        the neurons of each session, 1 <= n[s] <= N_max
 *   w_off[S]    element offset of the session's [n_s][P] row-major matrix from the base pointer `w` (of w_elems elements)
 *   b_off[S]    the same for its bias from `bias` (of b_elems elements; fp32 always); unused where there is no bias
 * A sample whose session index is outside [0, S), or whose session's span leaves [0, w_elems) / [0, b_elems), is treated as n_s = 0:
 * nothing of that span is read or written.  The padded-side operand is [B*T][ld_pad] with the session's real channels in columns
 * [0, n_s); columns >= n_s are NEVER read (they enter every product as zeros, whatever they hold, NaN included).
 * dtype is the storage of the activations and the weights (MMFM_F32 / MMFM_BF16), accumulation is fp32; biases, dW and db are fp32.
 * Any P, n_s, T >= 1.  No allocation, no synchronisation, no memset, no atomics: every call is capturable and gives the same bits
 * for the same inputs.  Argument checks return -1 before any HIP call.
 *
 *   mmfm_session_reduce   y[b, t, p] = sum_{c < n_s} x_pad[b, t, c] W_s[c, p] (+ bias_s[p])              y: [B*T][ld_p], columns >= P not written
 *                         the read-in forward; without a bias, also the read-out's input gradient df = dpred . Wout
 *   mmfm_session_expand   y_pad[b, t, c] = sum_p f[b, t, p] W_s[c, p] (+ bias_s[c]) for c < n_s, exactly 0 for n_s <= c < N_max
 *                         (columns [N_max, ld_pad) are not written); the read-out forward
 *   mmfm_session_dw       dW_s[c, p] = sum_{b: sid[b] = s} sum_t a_pad[b, t, c] q[b, t, p]   at dw + w_off[s]   (d->w is not read)
 *                         db (or NULL): bias_from_pad = 0: db_s[p] = sum q[.., p] (read-in);  1: db_s[c] = sum a_pad[.., c] (read-out),
 *                         at db + b_off[s].  The spans of a session without a sample in the batch are not written.
 * mmfm_session_dw reads the grouping of samples from `runs` (DEVICE int32 [mmfm_session_runs_ints(B, S, chunk)], built by the host
 * from the session indices and staged with the inputs):
 *   [0] live chunk entries  [1] chunk  [2] mmfm_session_dw_chunks(B, S, chunk)  [3] B
 *   order[B]                the samples grouped by session
 *   {session, start, count, k} per chunk entry: samples order[start .. start + count) ; k = 1: the only chunk of its session (written
 *                           directly), k >= 2: the first of k consecutive chunks of its session, k = 0: a later one of them.
 * A session of several chunks writes one fp32 slab per chunk into the workspace and a second launch sums them in chunk order.
 * At most 64 distinct sessions per batch fit the table's capacity, min(B, ceil(B / chunk) + min(S, B, 64)) entries. */
#define MMFM_SESSION_LINEAR 1
typedef struct {
    int dtype;
    int B, T, P, N_max, S;
    int ld_pad;                  /* row stride of the padded-side operand, >= N_max */
    int ld_p;                    /* row stride of the P-side operand (y of _reduce, f of _expand, q of _dw), >= P */
    const int32_t* sid;
    const int32_t* n;
    const int64_t* w_off;
    const int64_t* b_off;
    const void* w; int64_t w_elems;
    const float* bias; int64_t b_elems;
} mmfm_session_desc;
int mmfm_session_reduce(const mmfm_session_desc* d, const void* x_pad, void* y, mmfm_stream stream);
int mmfm_session_expand(const mmfm_session_desc* d, const void* f, void* y_pad, mmfm_stream stream);
int mmfm_session_dw_chunks(int B, int S, int chunk);
int64_t mmfm_session_runs_ints(int B, int S, int chunk);
int64_t mmfm_session_dw_workspace(int B, int P, int N_max, int S, int chunk);
int mmfm_session_dw(const mmfm_session_desc* d, const void* a_pad, const void* q, const int32_t* runs, int chunk, float* dw, float* db,
                    int bias_from_pad, void* workspace, int64_t workspace_bytes, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- span packing (sparse session all-reduce)
 * Copies a list of spans between a flat fp32 buffer G and a packed staging buffer, so that data parallelism all-reduces the session
 * layers a step touched in ONE collective instead of the whole session block.  MMFM_SPAN_PACK is the feature macro for the two exports
 * (MMFM_VERSION stays, as for MMFM_NULL_BIAS: no existing struct or kernel changed).
 *
 * table: DEVICE int64 [>= n_spans][4], 8-byte aligned, one row {g_off, s_off, len, live} per span, in elements.  The table is data:
 * the launch geometry depends on nothing it holds (a captured launch serves any table of the same n_spans), and rows beyond n_spans
 * are not read.
 *   mmfm_span_gather    stage[s_off .. s_off + len) = live ? G[g_off .. g_off + len) : 0
 *                       A span with live == 0 is NEVER loaded from G (its bytes may be anything, NaN included): zeros are stored.
 *   mmfm_span_scatter   G[g_off .. g_off + len) = stage[s_off .. s_off + len)   for every span, whatever `live` says
 * A row with len <= 0 or a negative offset is skipped.  The spans must not overlap in the buffer that is written; keeping them inside
 * both buffers is the caller's part (the table builder of ops.py checks it on the host).
 * A span whose two addresses agree modulo 16 bytes moves in 16-byte accesses over its aligned interior and element accesses over the at
 * most three elements of its head and of its tail; one whose addresses disagree moves element by element.  The work is cut into chunks
 * of MMFM_SPAN_CHUNK elements and the workgroups stride over all (span, chunk) pairs in table order: one long span and many short ones
 * both fill the device.  Exactly one lane stores each element, nothing outside the named ranges is written; no atomics, no
 * allocation, no synchronisation (capturable).  n_spans == 0 returns 0 without a launch.
 * Argument checks (NULL pointers, a misaligned table or buffer, n_spans outside [0, MMFM_SPAN_MAX]) return -1 before any HIP call: a
 * machine without a GPU answers them. */
#define MMFM_SPAN_PACK 1
#define MMFM_SPAN_CHUNK 4096
#define MMFM_SPAN_MAX 65536
int mmfm_span_gather(const float* G, float* stage, const int64_t* table, int n_spans, mmfm_stream stream);
int mmfm_span_scatter(const float* stage, float* G, const int64_t* table, int n_spans, mmfm_stream stream);

/* ---------------------------------------------------------------------------------- evaluation metrics
 * utils/utils.py:107-115 (metrics_list "r2" = torcheval R2Score per series; trainer/base.py:252-262 calls it for 50
 * neurons x every trial on the host):  out[g*C + c] = 1 - sum_s (y-p)^2 / sum_s (y - mean_s y)^2 over the S elements
 * y = gt[g*gs[0] + s*gs[1] + c*gs[2]] (element strides, so transposed / sliced views need no copy), fp64 sums.
 * A constant series gives -inf / nan like the reference; the caller masks invalids (np.ma.masked_invalid). */
int mmfm_r2_series(const float* gt, const int64_t* gt_strides, const float* pred, const int64_t* pred_strides,
                   int G, int S, int C, float* out, mmfm_stream stream);
/* utils/eval_utils.py:1051-1119 (neg_log_likelihood, bits_per_spike): rates, spikes fp32 [R][N] (R = trials x bins);
 * out[0] = bits per spike, out[1] = nll(model), out[2] = nll(null = per-neuron mean rate), out[3] = total spikes.
 * rates == 0 -> 1e-9 as upstream; NaN spikes are not supported (upstream masks them). */
int64_t mmfm_bits_per_spike_workspace(int64_t R, int N);
int mmfm_bits_per_spike(const float* rates, const float* spikes, int64_t R, int N, float* out,
                        void* workspace, int64_t workspace_bytes, mmfm_stream stream);
/* utils/eval_utils.py:846-851 (spiking_activity_recon_eval: bits_per_spike on each neuron's own slice, N host calls
 * upstream): out[n] = bits per spike of neuron n against ITS mean rate, all N in one pass.  A silent neuron gives
 * inf / nan like upstream (which then records NaN). */
int64_t mmfm_bits_per_spike_neurons_workspace(int64_t R, int N);
int mmfm_bits_per_spike_neurons(const float* rates, const float* spikes, int64_t R, int N, float* out,
                                void* workspace, int64_t workspace_bytes, mmfm_stream stream);


/* ---------------------------------------------------------------------------------- row-owner fused kernels (bf16, width 256)
 * Throughput-mode kernels in which a wavefront owns 32 token rows and keeps them in registers through a chain of ops while
 * the weights stream through LDS (csrc/rowchain.h).  They replace, for hidden_size 256 / inter_size 512 in bf16 mode, the
 * LayerNorm + nn.Linear pairs, the attention out_proj + residual, the whole MLP block and their autograd
 * (encoder_embeddings.py:106-116, decoder_embeddings.py:133-147, mm_utils.py:42-52,107-114,145-152, mm.py:290-292).
 *
 * mmfm_prep_weights: per training step (weights change) the LayerNorm affine is folded into the linear it feeds,
 *   Wp[n][k] = bf16(W[n][k] * gamma[k]),  WpT = Wp^T,  bp[n] = bias[n] + sum_k W[n][k] * beta[k]
 * so that  linear(layernorm(x)) = Wp . x_hat + bp  with  x_hat = (x - mean) * rstd.  gamma / beta / bias / Wp / WpT / bp / WpP / WpTP
 * may be NULL (plain bf16 copies / transposes of a weight).  `entries` is a DEVICE array; entry e covers blocks
 * [tile0, tile0 + ceil(N/32)); total_tiles = sum of ceil(N/32).
 * scalar_gain = 1 (a ScaleNorm-fed linear): gamma points to ONE float g (the ScaleNorm's gain) and beta is ignored:
 *   Wp = bf16(g * W),  WpT = Wp^T,  bp = bias,   so that  linear(scalenorm(x)) = Wp . x_hat + bp  with  x_hat = x / max(||x||, eps).
 * Bias-free linear (bias == NULL): under a LayerNorm (gamma / beta set) the prepared bias still exists, bp = W . beta - beta is folded
 *   into the linear whether or not the linear has a bias of its own; with scalar_gain = 1 nothing is left to add: pass bp = NULL (it is
 *   not written) and hand NULL on as the bias of the consuming kernel.  A non-NULL bp there is written as zeros. */
typedef struct {
    const float* W;          /* [N][K] fp32 master weight */
    const float* gamma;      /* [K] or NULL */
    const float* beta;       /* [K] or NULL */
    const float* bias;       /* [N] or NULL */
    void* Wp;                /* bf16 [N][K] or NULL */
    void* WpT;               /* bf16 [K][N] or NULL */
    float* bp;               /* fp32 [N] or NULL */
    int N, K;
    int tile0;
    int scalar_gain;         /* 0: gamma / beta per k (LayerNorm);  1: gamma[0] is a scalar gain for every k, no beta (ScaleNorm) */
    void* WpP;               /* bf16 [N][K] or NULL: Wp with the 8-byte units of every aligned 32-byte group of a row in the order
                                0, 2, 1, 3 ("unit-permuted": the order in which an MFMA accumulator tile, used as the next product's
                                operand, holds its k index - rowchain.h).  LDS-DMA cannot permute on the way in, so the kernels that
                                multiply such operands read these copies: mmfm_mlp_fwd's w_down */
    void* WpTP;              /* bf16 [K][N] or NULL: WpT unit-permuted along N: mmfm_mlp_bwd's w_up_t.
                                The permutation acts on aligned groups of 16 elements: WpP requires K % 16 == 0 and WpTP requires
                                N % 16 == 0 (a ragged last group has no permuted position inside its row: the kernel leaves those
                                elements unwritten rather than spill into the next row) */
} mmfm_prep_entry;
int mmfm_prep_weights(const mmfm_prep_entry* entries, int n_entries, int total_tiles, mmfm_stream stream);

/* y[R][N] = epi( pro(x)[R][K] . w[N][K]^T ), bf16 storage, fp32 accumulate; K in {256, 512, 768}, N % 32 == 0.
 *   ln = 1 (K = 256): pro(x) = x_hat = (x - mean(x)) * rstd(x) per row (statistics in fp32); x_hat (bf16 [R][256]) and rstd
 *                      (fp32 [R]) are written when non-NULL (the backward's saved tensors); w / bias are the PREPARED Wp / bp.
 *   ln = 2 (K = 256): ScaleNorm: pro(x) = x_hat = x * rstd, rstd = 1 / max(||x||, eps), saved NEGATED for a clamped row (as
 *                      mmfm_scalenorm_fwd's rinv); w / bias prepared with mmfm_prep_entry.scalar_gain = 1.
 *   epilogue: + bias[n], + residual[m*ldr + n], store.
 *   bias == NULL adds nothing, in every mode and on both rings (the kernels keep the bias in LDS; a NULL one is staged as zeros, so
 *                      the result is bit-identical to passing a zero vector).
 *   ln_bwd = 1 (N = 256): v = x . w^T is d(x_hat) of a LayerNorm whose output fed the forward linear (w = WpT of it) and
 *                      y = residual + bwd_rstd * (v - mean(v) - bwd_xhat * mean(v * bwd_xhat))   (residual = running gradient or NULL).
 *   ln_bwd = 2 (N = 256): the same for a ScaleNorm (x_hat / rstd saved by ln = 2):
 *                      y = residual + |bwd_rstd| * (v - bwd_xhat * sum(v * bwd_xhat)),  the sum dropped where bwd_rstd < 0 (clamped). */
typedef struct {
    int64_t R;
    int K, N;
    const void* x; int ldx;
    const void* w; int ldw;
    const float* bias;
    int ln; float eps;
    void* xhat; float* rstd;
    const void* residual; int ldr;
    void* y; int ldy;
    int stream_out;          /* 1: non-temporal stores of y */
    int rotate;              /* 1: workgroups start at different weight tiles (spreads the concurrent L2 reads) */
    int ln_bwd;
    const void* bwd_xhat; const float* bwd_rstd;
} mmfm_rowgemm_desc;
int mmfm_rowgemm(const mmfm_rowgemm_desc* d, mmfm_stream stream);
/* The form a dX + norm-backward launch (ln_bwd != 0; mmfm_rowgemm, or mmfm_rowgemm_groups backward) over R rows takes at this K, as the
 * dispatcher decides it at this moment (it reads MMFM_ROWGEMM_LNBWD_WG at every launch): 2 = the kernel of which two workgroups share a
 * CU (K = 512 / 768 only), 1 = the one-workgroup kernels.  Both forms write bit-identical results.  A query: no launch, no error state. */
int mmfm_rowgemm_lnbwd_form(int64_t R, int K);

/* The row-owner linear over up to MMFM_ROWGEMM_MAX_GROUPS weight sets in ONE launch (the context side of cross-attention: every
 * decoder layer projects the same normalised context rows to its keys / values, and their dX products sum into one gradient).
 *   ln_bwd == 0 (grouped forward; ln = 1 or 2, K = 256, N in {64, 128, 256, 512, 1024}, groups * N <= 2560):
 *       x_hat = norm(x[0]) once per row (written to xhat / rstd when non-NULL), then for every group g
 *       y[g][R][N] = x_hat . w[g][N][K]^T + bias[g]        each y[g] bit-identical to mmfm_rowgemm(ln, x[0], w[g], bias[g]).
 *   ln_bwd = 1 or 2 (grouped dX + norm backward; N = 256, K = 256 or 512 per group):
 *       v = sum_g x[g][R][K] . w[g][256][K]^T   (w[g] = WpT of group g's forward linear, fp32 accumulation over all groups)
 *       y[0] = residual + norm'(v)               exactly mmfm_rowgemm's ln_bwd epilogue on the summed product.
 * Operands, outputs and weights of all groups share ldx / ldy / ldw; every tensor stays below 2 GiB, and the groups' weight matrices
 * lie within 2 GiB of each other (they are slices of one prepared-weight tensor).
 * MMFM_ROWGEMM_MAX_GROUPS is the feature macro for this export (MMFM_VERSION stays, as for MMFM_NULL_BIAS: no existing struct changed). */
#define MMFM_ROWGEMM_MAX_GROUPS 8
typedef struct {
    int64_t R;
    int K, N;                /* per group */
    int groups;              /* 1 .. MMFM_ROWGEMM_MAX_GROUPS */
    const void* x[MMFM_ROWGEMM_MAX_GROUPS]; int ldx;     /* forward: x[0] only */
    const void* w[MMFM_ROWGEMM_MAX_GROUPS]; int ldw;
    const float* bias[MMFM_ROWGEMM_MAX_GROUPS];          /* forward; NULL adds nothing */
    void* y[MMFM_ROWGEMM_MAX_GROUPS]; int ldy;           /* backward: y[0] only */
    int ln; float eps;
    void* xhat; float* rstd;
    const void* residual; int ldr;                       /* backward only */
    int stream_out, rotate;
    int ln_bwd;
    const void* bwd_xhat; const float* bwd_rstd;
} mmfm_rowgemm_groups_desc;
int mmfm_rowgemm_groups(const mmfm_rowgemm_groups_desc* d, mmfm_stream stream);

/* The MLP block in one launch (mm_utils.py:42-52 behind ln2, encoder_embeddings.py:114, decoder_embeddings.py:145):
 *   fwd:  y = x + dropout( down( gelu_erf( up( layernorm(x) ) ) ) )        the 512-wide intermediate never leaves the CU
 *         (gelu stands for the activation `act` throughout: GELU unless the trailing field says otherwise)
 *         w_up / b_up are the prepared (gamma / beta folded) [512][256] / [512]; w_down = bf16 [256][512], UNIT-PERMUTED
 *         (mmfm_prep_entry.WpP of down_proj: the weights reach LDS by DMA, which cannot permute); x_hat / rstd are written for the backward.
 *   bwd:  recomputes u = up(x_hat) and g = gelu(u) from the saved x_hat instead of loading them, and produces
 *         t1 = dropout'(dy)                      [R][256]   (operand of dW_down = t1^T g, db_down = colsum t1)
 *         g                                      [R][512]
 *         du = (t1 . W_down) * gelu'(u)          [R][512]   (operand of G_up = du^T x_hat, db_up = colsum du)
 *         dx = dy + LayerNorm'(du . Wp_up)       [R][256]   (LayerNorm backward in registers; needs w_up_t = Wp_up^T UNIT-PERMUTED =
 *                                                            mmfm_prep_entry.WpTP of up_proj, w_down_t = W_down^T)
 *   Weight / LayerNorm-parameter gradients then follow from mmfm_gemm (dW slabs) + mmfm_ln_linear_grad.
 *   Bias-free linears (mlp_bias: false): b_down may be NULL (nothing is added to Y).  b_up may be NULL only with scalenorm = 1; under a
 *   LayerNorm b_up is the prepared W_up . beta and is always present (a NULL one is an argument error).  The backward kernels (one-launch
 *   and front half) read the same b_up the forward read, so the recomputed u follows the same rule; they never read b_down.
 *   du only (MMFM_MLP_DX_ONLY): the front half (dx == NULL) with t1 == NULL && g == NULL writes du and nothing else - for a caller that
 *   wants neither dW_down nor G_up (both projections frozen), the only readers of t1 and g.  du is bit for bit what the full front half
 *   writes.  t1 and g are both NULL or both set; one NULL, or NULLs with dx != NULL, is an argument error and nothing is launched. */
typedef struct {
    int64_t R;
    const void* x; int ldx;           /* fwd: residual stream in (bf16 [R][256]) */
    float eps;
    const void* w_up; const float* b_up;
    const void* w_down; const float* b_down;      /* w_down: unit-permuted (WpP) */
    mmfm_dropout drop;
    void* y; int ldy;
    void* xhat; float* rstd;          /* fwd: out;  bwd: in */
    /* backward only */
    const void* dy; int lddy;
    const void* w_down_t;             /* bf16 [512][256] */
    const void* w_up_t;               /* bf16 [256][512] (prepared, unit-permuted: WpTP) */
    void* t1; void* g; void* du;
    void* dx; int lddx;               /* dx == NULL: front half only - t1, g, du are written and the call returns; rstd / w_up_t are not read.
                                         The caller finishes with mmfm_rowgemm(x = du, w = WpT of up_proj, K = 512, residual = dy, ln_bwd) */
    int rotate;                       /* 1: workgroups start at different intermediate tiles (spreads the concurrent L2 reads) */
    int scalenorm;                    /* 0: ln2 is a LayerNorm;  1: a ScaleNorm (fwd: x_hat = x / max(||x||, eps), rstd saved as by
                                         mmfm_rowgemm ln = 2, w_up / b_up prepared with scalar_gain = 1).  The one-launch backward (dx != NULL)
                                         refuses it: the front half + mmfm_rowgemm(ln_bwd = 2) is the ScaleNorm backward */
    int act;                          /* MMFM_MLP_GELU (0, the zero-initialised default), _RELU, _SIGMOID or _GELU_TANH: the activation of
                                         the forward, of g and of du = (t1 . W_down) * act'(u) in every backward mode */
    float act_beta;                   /* MMFM_MLP_SIGMOID only: u * sigmoid(act_beta * u); 0 there means 1 (silu) */
} mmfm_mlp_desc;
int mmfm_mlp_fwd(const mmfm_mlp_desc* d, mmfm_stream stream);
int mmfm_mlp_bwd(const mmfm_mlp_desc* d, mmfm_stream stream);

/* Gradients of a LayerNorm-fed linear from the reduced weight-gradient GEMM against x_hat:
 *   Gdb = [ G[N][K] | db[N] ],  G = dY^T x_hat,  db = colsum dY   (one mmfm_gemm + mmfm_reduce_slabs)
 *   dW[n][k] = gamma[k] * G[n][k] + db[n] * beta[k];   dbias = db;
 *   dgamma[k] (+)= sum_n W[n][k] * G[n][k];   dbeta[k] (+)= sum_n W[n][k] * db[n]      (accumulate_ln selects +=)
 * No per-row reduction is needed for the LayerNorm parameters.  Deterministic.
 * dbias == NULL (a bias-free linear): nothing is written for it.  Gdb keeps its trailing db block - dW and dbeta need db because beta
 * is folded into the linear.
 * workspace: mmfm_ln_linear_grad_workspace(K) bytes, ZEROED once before its first use (partial rows + arrival tickets that
 * the kernel re-arms itself); one workspace per concurrently running launch. */
int64_t mmfm_ln_linear_grad_workspace(int K);
int mmfm_ln_linear_grad(const float* Gdb, const float* W, const float* gamma, const float* beta, int N, int K,
                        float* dW, float* dbias, float* dgamma, float* dbeta, int accumulate_ln,
                        void* workspace, int64_t workspace_bytes, mmfm_stream stream);
/* The same for a ScaleNorm-fed linear (scalar gain g, one float; Gdb from x_hat = x / max(||x||, eps)):
 *   dW = g * G;   dbias = db;   dg (+)= sum_{n,k} W[n][k] * G[n][k]      (accumulate selects +=)
 * dbias == NULL (a bias-free linear): nothing is written for it AND the trailing db block of Gdb is never read: Gdb may then be
 * just G[N][K] (N * K floats), from a weight-gradient GEMM launched without colsum.
 * Deterministic (per-block partials summed in a fixed order by the last block).  Same workspace (size, zeroing, one per concurrent
 * launch) as mmfm_ln_linear_grad. */
int mmfm_sn_linear_grad(const float* Gdb, const float* W, const float* g, int N, int K, float* dW, float* dbias, float* dg,
                        int accumulate, void* workspace, int64_t workspace_bytes, mmfm_stream stream);

/* ------------------------------------------------------------------ MT19937 jump-ahead (HOST memory, no device, no HIP call)
 * Moves an MT19937 state (the engine of torch's CPU generator) on by n 32-bit outputs without drawing them: what the masker's
 * discarded [B, T, N] corruption draws (models/masker.py:157-163 under mm.py:267) amount to.  Works in a process that never
 * initialised HIP.
 *   state624: the 624 state words, regenerated in place as the engine does;
 *   consumed: in/out, words of the current block already handed out, 0..624 (624: the next output regenerates first; a freshly
 *             seeded engine, which has handed out nothing of its seed block, is 624 too);
 *   n:        outputs to skip.  Afterwards consumed is 1..624 whenever a block boundary was crossed.
 * The result is bit-identical to n real draws.  Long moves jump whole blocks through t^(624 D) mod phi (phi: the characteristic
 * polynomial, found once per process; one polynomial per block count D is cached), short ones step the recurrence. */
int mmfm_mt19937_jump(uint32_t* state624, int32_t* consumed, uint64_t n);
/* Drops the cached polynomials (the next long jump pays for phi and its power again): cold-cost measurements. */
int mmfm_mt19937_jump_reset(void);

/* ------------------------------------------------------------------ MT19937 on the device: the draws whose values ARE read
 * The outputs of the same engine, generated on the GPU bit for bit as torch's CPU generator hands them out: output i of the
 * position (state624, consumed) is the tempered word i, u_i = float(out_i & 0xFFFFFF) * 2^-24 is torch.rand's value and
 * u_i < float(p) is torch.bernoulli's, element i of a row-major fp32 tensor taking output i.  The host generator is not touched: the
 * caller moves it on with mmfm_mt19937_jump.
 *   state624, consumed: HOST values with mmfm_mt19937_jump's meaning (624: regenerate first / freshly seeded), read during the call
 *             and carried to the device as a launch argument: the caller may reuse the array when the call returns;
 *   streams:  0 = the library's choice (a power of two, at least 64 blocks a run, at most 256 runs), 1 .. MMFM_MT_MAX_STREAMS forces it.  The n outputs are cut into `streams` runs of `blocks`
 *             whole 624-output blocks, one workgroup each (mmfm_mt_plan names the cut: run s covers outputs [s * blocks * 624,
 *             min(n, (s + 1) * blocks * 624)), trailing runs may be empty); run s > 0 starts from a state that is a jump of whole
 *             blocks - applied on the device through t^(624 D) mod phi, in a doubling tree over ceil(log2 streams) polynomials whose
 *             bit lists are uploaded once per block count D.  The result does not depend on `streams`.
 *   workspace: mmfm_mt_workspace(n, streams) bytes of device memory, 16-byte aligned, contents arbitrary (n: outputs of one draw, for
 *             mmfm_mt_corrupt B * T * N; the size serves all three entries).
 * mmfm_mt_uniform    out[i] = u of output skip + i, i < n (fp32).
 * mmfm_mt_bernoulli  out[i] = (u of output skip + i) < p (uint8 0 / 1); p in [0, 1].
 * mmfm_mt_corrupt    one masker call (models/masker.py), draws u1, u2, u3 = outputs i, BTN + i, 2 BTN + i of element i:
 *                      z = cm(b,t,n) & (u1 < zero_ratio);  dst = z ? 0 : src;  m = max(dst) over all elements, NaN if any NaN survives
 *                      (torch.max);  dst = m * u3 (one fp32 multiply) where cm & !z & (u2 < random_ratio).
 *                    src / dst fp32 [B][T][N] contiguous (dst may be src), cm a strided uint8 mask as for mmfm_stage_masked (any
 *                    stride may be 0), B * T * N < 2^31.  m is found by a first pass that regenerates u1 alone (per-run maxima in the
 *                    workspace, reduced in a fixed order by every workgroup of the second); the pass is skipped where no element can
 *                    take noise (random_ratio == 0 or zero_ratio >= 1).
 * Argument checks (null pointers, consumed outside 0..624, n == 0 or beyond 2^62, p / ratios outside [0, 1] or NaN, streams, negative
 * strides, a short or misaligned workspace) return -1 before any HIP call.  The first call that needs a block count D computes its polynomial
 * (host, tens of ms) and uploads it (one allocation, one synchronous copy; at most MMFM_MT_TABLES tables per device are kept); after
 * that no call allocates or synchronises.  No atomics, no memset: the same bits on every call.
 * MMFM_MT_DEVICE is the feature macro for the exports (MMFM_VERSION stays, as for MMFM_LOSS_ELEM). */
#define MMFM_MT_DEVICE 1
#define MMFM_MT_MAX_STREAMS 1024
#define MMFM_MT_TABLES 64
/* pure (no HIP call): the cut of n outputs; streams = 0 picks it.  Returns -1 for n == 0 or streams outside 0..MMFM_MT_MAX_STREAMS. */
int mmfm_mt_plan(uint64_t n, int streams, int32_t* out_streams, int64_t* out_blocks);
int64_t mmfm_mt_workspace(uint64_t n, int streams);
int mmfm_mt_uniform(const uint32_t* state624, int32_t consumed, uint64_t skip, uint64_t n, float* out, int streams,
                    void* workspace, int64_t workspace_bytes, mmfm_stream stream);
int mmfm_mt_bernoulli(const uint32_t* state624, int32_t consumed, uint64_t skip, uint64_t n, float p, uint8_t* out, int streams,
                      void* workspace, int64_t workspace_bytes, mmfm_stream stream);
int mmfm_mt_corrupt(const uint32_t* state624, int32_t consumed, int B, int T, int N, const float* src, const uint8_t* cm,
                    int64_t sb, int64_t st, int64_t sn, float zero_ratio, float random_ratio, float* dst, int streams,
                    void* workspace, int64_t workspace_bytes, mmfm_stream stream);

#ifdef __cplusplus
}
#endif
#endif
