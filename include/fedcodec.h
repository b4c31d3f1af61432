/* fedcodec.h — C ABI of the MI355X-native gradient codec (libfedcodec.so, gfx950).
 *
 * Replaces the NumPy kernels inside OpenMSFTL's ftl/compression + FedAVG hot path:
 *   Compression.compress          ftl/compression/compression.py:23-77
 *     'top'              -> fc_topk_encode (+ fc_topk_encode_exact)   compression.py:31-37
 *     'rand'             -> fc_topk_encode (key_mode = PHILOX, native) or
 *                           fc_mask_encode (host permutation mask, parity)  compression.py:39-45
 *     'dropout-biased'   -> fc_mask_encode (codec = DROPOUT_BIASED)   compression.py:47-53
 *     'dropout-unbiased' -> fc_mask_encode (codec = DROPOUT_UNBIASED) compression.py:55-60
 *     dense result       -> fc_decode_dense
 *   Aggregator.aggregate_grads G build   aggregation.py:61-63   -> fc_decode_accumulate
 *   GAR.weighted_average / FedAvg        gar.py:32-46, 53-56    -> fc_decode_accumulate /
 *                                                                  fc_weighted_sum_dense
 *   flatten_params / client delta        model_helper.py:11-35,
 *                                        client.py:44,52-53     -> fc_flat_stage
 *   Aggregator.__merge_gradient          aggregation.py:80-93   -> fc_decode_accumulate /
 *                                                                  fc_weighted_sum_dense (w=1)
 *                                                                  + fc_div_scalar
 * The reference has no FFI of its own (100 % Python): these entry points are
 * what its Python layer binds through ctypes.
 *
 * Conventions: every pointer is a DEVICE pointer unless stated; buffers are caller-owned;
 * calls are stream-ordered and asynchronous; nothing allocates (scratch lives in the caller's
 * workspace); return 0 on success, <0 on argument / HIP errors (fc_last_error() explains,
 * thread-local).  Device-side outcomes (e.g. the sampled bracket missing) are reported in the
 * packet header's `status`, read by the host after the stream is synchronised.
 *
 * Concurrency: every entry point may run beside any other kernel, on any stream.  Two
 * launches wait in-kernel (bounded) for a bracket their own sample workgroups publish: k_fused_mag
 * (fc_topk_encode with key_mode MAGNITUDE and 0 < k < n, fc_topk_encode_dense) and k_fused64
 * (fc_topk_dense_f64_sampled).  Two of them on two streams of one device could stall each other
 * (each XCD dispatches the two grids in its own order), so the library queues each one after the
 * device's previous one: an event it owns completes with every such launch, and a launch on
 * another stream first waits for it.  A launch into a stream being captured (hipGraph) is not
 * ordered; bracket the graph's launch with fc_fused_order_begin / fc_fused_order_end.  All other
 * kernels synchronise only through last-arriver tickets (no workgroup waits for another).
 */
#ifndef FEDCODEC_H_
#define FEDCODEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fc_stream_t; /* hipStream_t */

/* ABI history: 2 = per-chunk quarter offsets (qoff); 3 = uint16 chunk-local packet indices;
 * 4 = fc_topk_encode_dense's packet is scratch (no entries; header format FC_FMT_DENSE, which
 * the decode entry points must not be given: they trust the caller's format argument).  A C
 * caller built against 3 that decoded that packet must check this version. */
#define FC_ABI_VERSION 4

/* return codes */
#define FC_OK 0
#define FC_ERR_ARG (-1)
#define FC_ERR_HIP (-2)
#define FC_ERR_WORKSPACE (-3)

/* packet header status (device-written) */
#define FC_STATUS_OK 0
#define FC_STATUS_RETRY_EXACT 1   /* sampled bracket missed: call fc_topk_encode_exact */
#define FC_STATUS_OVERFLOW 2      /* more entries than the packet capacity */
#define FC_STATUS_TIMEOUT 3       /* a bounded device spin expired (never expected) */

/* codecs (compression_function) */
#define FC_CODEC_TOP 1
#define FC_CODEC_RAND 2
#define FC_CODEC_DROPOUT_BIASED 3
#define FC_CODEC_DROPOUT_UNBIASED 4
#define FC_CODEC_QSGD 5      /* opt-in: the reference raises NotImplementedError (:62-64)    */
#define FC_CODEC_SIGN 6      /* opt-in, no reference counterpart: scaled sign (fc_sign_encode) */

/* key sources for fc_topk_encode */
#define FC_KEY_MAGNITUDE 0   /* |g| (top-k) */
#define FC_KEY_PHILOX 1      /* Philox4x32-10 word per element (native rand-k) */

/* packet formats */
#define FC_FMT_IDXVAL 0      /* uint16 idx[] (chunk-local, ascending) + float val[] */
#define FC_FMT_BITMAP 1      /* uint32 bitmap[ceil(N/8192)*256] + float val[] */
#define FC_FMT_QSGD 2        /* packed W-bit codes (sign | level), fc_qsgd_code_words */
#define FC_FMT_DENSE 3       /* header of fc_topk_encode_dense: the dense q is the product;
                                idx/val/cnt/qoff are scratch (not a decodable packet) */
#define FC_FMT_SIGN 4        /* uint32 word[fc_sign_words(n)] of sign bits + the scale in hdr.p */

/* Slotted packet layout: the gradient is cut into chunks of FC_CHUNK elements; chunk c's
 * entries (ascending index order) live at [c*FC_CHUNK, c*FC_CHUNK + cnt[c]) of idx/val (and
 * its bitmap words at [c*256, c*256+256)).  idx holds the CHUNK-LOCAL index (uint16, the
 * element is c*FC_CHUNK + idx): 6 bytes per entry instead of 8 (ABI 3).  Every chunk is encoded by an independent
 * workgroup — no global scan — so buffers are sized fc_packet_capacity(n) entries while only
 * the listed entries are written or read.
 * FC_FMT_IDXVAL packets also carry qoff[c] (uint64 per chunk): the slot positions where the
 * chunk's four quarters (FC_CHUNK/4 elements each) begin — quarter 1, 2, 3 in bits 0-15,
 * 16-31, 32-47 — and cnt[c] in bits 48-63, so a decoder can hand each quarter to its own wave
 * (fc_decode_accumulate requires it). */
#define FC_CHUNK 8192        /* elements per chunk */
#define FC_QUARTER (FC_CHUNK / 4)

/* Device-resident packet header (96 bytes). */
typedef struct fc_packet_hdr {
  uint64_t thresh;      /* T64: entry kept iff (key<<index_bits | index) >= thresh    */
  uint64_t lower;       /* L64: every element with comp >= lower is listed             */
  uint32_t n;           /* gradient length                                             */
  uint32_t k;           /* coordinates kept by the codec (top/rand)                    */
  uint32_t n_entries;   /* entries listed (sum of cnt; >= k: sampled-bracket slack)    */
  uint32_t index_bits;  /* IB = max(1, ceil(log2 n))                                   */
  uint32_t codec;       /* FC_CODEC_*                                                  */
  uint32_t status;      /* FC_STATUS_*                                                 */
  uint32_t n_definite;  /* diagnostics: elements above the bracket                     */
  uint32_t n_cand;      /* diagnostics: elements inside the bracket                    */
  uint64_t seed;        /* Philox key (native RNG modes)                               */
  uint64_t offset;      /* Philox counter high words                                   */
  double p;             /* dropout probability (unbiased scale 1/p applied at decode)  */
  uint32_t chunk;       /* FC_CHUNK                                                    */
  uint32_t format;      /* FC_FMT_*                                                    */
  uint32_t key_mode;    /* FC_KEY_* (top/rand)                                         */
  uint32_t reserved[3];
} fc_packet_hdr;

/* One packet as seen by the decoders (host- or device-resident array element, 56 bytes). */
typedef struct fc_packet_view {
  const void* idx;              /* FC_FMT_IDXVAL: uint16 chunk-local indices; FC_FMT_QSGD: uint32 codes */
  const float* val;
  const uint32_t* bitmap;       /* FC_FMT_BITMAP; FC_FMT_SIGN: the words */
  const uint32_t* cnt;          /* ceil(N/FC_CHUNK) entries per chunk   */
  const fc_packet_hdr* hdr;
  const uint64_t* qoff;         /* FC_FMT_IDXVAL: quarter offsets per chunk (see above) */
  float weight;                 /* FedAVG weight w_i (gar.py:37-44)     */
  uint32_t reserved;
} fc_packet_view;

int fc_abi_version(void);
const char* fc_last_error(void);

/* ---- sizes ------------------------------------------------------------------------- */
uint64_t fc_num_chunks(uint64_t n);
size_t fc_workspace_bytes(uint64_t n);        /* scratch for one encoder (one stream)   */
uint64_t fc_packet_capacity(uint64_t n);      /* idx/val entries: ceil(n/FC_CHUNK)*FC_CHUNK */
/* zero a freshly allocated workspace once (self-cleaning afterwards) */
int fc_workspace_init(void* ws, size_t ws_bytes, fc_stream_t stream);

/* ---- encode: top-k / native rand-k (compression.py:31-45) ---------------------------
 * Single streaming read of g: a sampled bracket [t_lo, t_hi] is estimated from a
 * stratified sample, every element with key >= t_lo is compacted in index order into its
 * chunk's slot (one launch, independent workgroups), then the exact k-th composite key is
 * resolved from the bracket's candidates.  hdr->status == FC_STATUS_RETRY_EXACT means the
 * bracket missed (adversarial / tie-heavy data): call fc_topk_encode_exact with the same
 * arguments.  capacity >= fc_packet_capacity(n); cnt and qoff have fc_num_chunks(n) words
 * (qoff may be NULL: not written; fc_decode_accumulate then folds the packet by scanning each
 * chunk's whole slot range per quarter, correct but slower). */
int fc_topk_encode(const float* g, uint64_t n, uint64_t k, int key_mode, uint64_t seed,
                   uint64_t offset, uint16_t* idx, float* val, uint64_t capacity,
                   uint32_t* cnt, uint64_t* qoff, fc_packet_hdr* hdr, void* ws, size_t ws_bytes,
                   fc_stream_t stream);
/* ---- top-k straight to the dense result (compression.py:31-37 returns q, not a packet) --
 * The fc_topk_encode pipeline (magnitude keys) whose compaction pass also streams
 * q = zeros_like(g); q[listed] = g into `dense` (n floats, 16-B aligned); the resolve zeroes
 * the slack entries once T64 is known.  q is the product: the packet buffers are scratch (the
 * entries are written only for chunks the resolve has to re-read) and the header's format is
 * FC_FMT_DENSE (thresh / status valid; not decodable).  If the header reports
 * FC_STATUS_RETRY_EXACT, `dense` is not valid: re-encode with fc_topk_encode_exact (a full
 * packet) and fc_decode_dense.  Needs 0 < k < n. */
/* fc_topk_encode_decode: the packet encode of fc_topk_encode (key_mode MAGNITUDE, 0 < k < n,
 * qoff required) AND its dense decode into out (float32[n], 16-B aligned), with the resolve's
 * gather and finish inside the decode launch (k_fused_mag -> k_beta -> k_decode_res): the packet
 * (entries, counts, quarter offsets, header with T64) equals fc_topk_encode's byte for byte and
 * out equals fc_decode_dense of it.  Replaces compression.py:31-37 + the caller's use of q.
 * Header status FC_STATUS_RETRY_EXACT: call fc_topk_encode_exact, then fc_decode_dense. */
int fc_topk_encode_decode(const float* g, uint64_t n, uint64_t k, uint16_t* idx, float* val,
                          uint64_t capacity, uint32_t* cnt, uint64_t* qoff, fc_packet_hdr* hdr,
                          void* ws, size_t ws_bytes, float* out, fc_stream_t stream);
int fc_topk_encode_dense(const float* g, uint64_t n, uint64_t k, uint16_t* idx, float* val,
                         uint64_t capacity, uint32_t* cnt, uint64_t* qoff, fc_packet_hdr* hdr,
                         void* ws, size_t ws_bytes, float* dense, fc_stream_t stream);
/* ---- top-k with error feedback (residual accumulation; opt-in, no reference counterpart) --
 * compression.py:31-37 drops the N - k unselected coordinates for good; with error feedback
 * the client adds them to its next gradient.  One streaming pass over g and the residual:
 *   a  = fl32(g + res_in)                       one IEEE fp32 add per element
 *   packet                                      exactly what fc_topk_encode(a, ...) writes (keys
 *                                               on |a|, highest index first in a tie, NaN largest,
 *                                               val = a[idx], cnt, qoff, header: codec TOP, format
 *                                               IDXVAL, T64, L64): decoders take it unchanged
 *   res_out[i] = +0.0f at the k selected coordinates (also for a selected NaN or +-inf, where
 *                a - q would be NaN), a[i] everywhere else (an unselected -0.0 stays -0.0)
 * g and res_in are never written; res_out (float32[n]) must not overlap either.  All three are
 * 16-B aligned.  Needs 0 < k < n.  Launches: sample, compaction, resolve — the unfused chain,
 * no kernel that waits in-kernel for another workgroup, so no fc_fused_order_* handling.
 * Header status FC_STATUS_RETRY_EXACT: the packet AND res_out are not valid; run the fallback
 *   fc_ef_sum(g, res_in, res_out) -> fc_topk_encode_exact(res_out, ...) -> fc_ef_clear(pkt, res_out)
 * which is also the form for k == 0 (empty packet, res_out = a) and k == n (res_out all +0).
 * fc_ef_sum:   res_out = fl32(g + res_in)  (same aliasing and alignment rules).
 * fc_ef_clear: +0.0f into res_out at every entry of the idx/val packet the decoders keep
 *   (composite >= T64); pkt: HOST pointer to one view (its hdr, cnt, idx, val on the device).
 * Argument errors (NULL, alignment, aliasing, k, capacity: FC_ERR_ARG; a short workspace:
 * FC_ERR_WORKSPACE) are reported before the GPU is touched. */
int fc_topk_encode_ef(const float* g, const float* res_in, float* res_out, uint64_t n, uint64_t k,
                      uint16_t* idx, float* val, uint64_t capacity, uint32_t* cnt, uint64_t* qoff,
                      fc_packet_hdr* hdr, void* ws, size_t ws_bytes, fc_stream_t stream);
int fc_ef_sum(const float* g, const float* res_in, float* res_out, uint64_t n, fc_stream_t stream);
int fc_ef_clear(const fc_packet_view* pkt, uint64_t n, float* res_out, fc_stream_t stream);
/* ---- batched top-k / native rand-k: M clients, one launch per pipeline stage ----------
 * The same fast path as fc_topk_encode for m gradients of equal length n, with the grid's
 * y dimension indexing the client: 4 launches for the whole batch instead of 4 per client,
 * so the small sampling / resolve stages of all clients overlap.  jobs: DEVICE array of m
 * fc_encode_job; ws: fc_workspace_bytes_batch(n, m) bytes, zeroed once with
 * fc_workspace_init.  Requires 0 < k < n (trivial k: fc_topk_encode).  A packet whose header
 * reports FC_STATUS_RETRY_EXACT is re-encoded with fc_topk_encode_exact, as for one client. */
typedef struct fc_encode_job {
  const float* g;        /* gradient, 16-B aligned                          */
  uint16_t* idx;         /* packet buffers (capacity >= fc_packet_capacity) */
  float* val;
  uint32_t* cnt;
  fc_packet_hdr* hdr;
  uint64_t seed;         /* Philox key / counter (FC_KEY_PHILOX)            */
  uint64_t offset;
  uint64_t* qoff;        /* quarter offsets per chunk (may be NULL)         */
} fc_encode_job;         /* 64 bytes */
size_t fc_workspace_bytes_batch(uint64_t n, int m);
int fc_topk_encode_batch(const fc_encode_job* jobs_dev, int m, uint64_t n, uint64_t k,
                         int key_mode, uint64_t capacity, void* ws, size_t ws_bytes,
                         fc_stream_t stream);
/* The same pipeline in two parts on the caller's stream (the same jobs and ws for both):
 * FC_PART_SAMPLE launches the bracket sample, which reads g and writes only the headers and
 * the workspace; FC_PART_FINISH launches the compaction and the exact resolve, which write the
 * packet buffers.  A caller that double-buffers the headers can therefore run the next
 * batch's sample while the previous packets are still being read (fc_decode_accumulate), and
 * order FC_PART_FINISH behind that fold.  part = FC_PART_SAMPLE | FC_PART_FINISH is
 * fc_topk_encode_batch. */
#define FC_PART_SAMPLE 1
#define FC_PART_FINISH 2
int fc_topk_encode_batch_part(const fc_encode_job* jobs_dev, int m, uint64_t n, uint64_t k,
                              int key_mode, uint64_t capacity, void* ws, size_t ws_bytes,
                              int part, fc_stream_t stream);
/* ---- batched top-k with error feedback: fc_topk_encode_ef for m clients ---------------
 * Client c: a_c = fl32(jobs[c].g + ef[c].res_in), one IEEE add per element; packet c is the one
 * fc_topk_encode_batch writes for a_c (so also fc_topk_encode_ef's, bit for bit); ef[c].res_out
 * is +0.0f at the k selected coordinates and a_c elsewhere.  Magnitude keys only: the jobs' seed
 * and offset are ignored (the headers carry 0).  Launches for the whole batch: pilot, sample,
 * compaction, two resolves; none waits in-kernel for another workgroup (last-arriver tickets
 * only), so there is no fc_fused_order_* handling.  ws: fc_workspace_bytes_batch(n, m), zeroed
 * once.  Needs 1 <= m <= 65535 and 0 < k < n.
 * Both tables are DEVICE memory, so the library cannot look inside them: 16-B alignment of every
 * g / res_in / res_out, their length n, and that no res_out overlaps any g, res_in or other
 * res_out of the batch are the caller's contract.  What the host can see (NULL tables, m, k,
 * capacity: FC_ERR_ARG; a short workspace: FC_ERR_WORKSPACE) is reported before the GPU is
 * touched.
 * A header with FC_STATUS_RETRY_EXACT: THAT client's packet and res_out are not valid; run
 * fc_ef_sum -> fc_topk_encode_exact -> fc_ef_clear for it alone.  Other clients are unaffected. */
typedef struct fc_ef_job {
  const float* res_in;   /* residual e (16-B aligned, n floats); never written            */
  float*       res_out;  /* new residual e'; must not overlap any g / res_in / res_out of the batch */
} fc_ef_job;             /* 16 bytes; entry c belongs to jobs[c] */
int fc_topk_encode_ef_batch(const fc_encode_job* jobs_dev, const fc_ef_job* ef_dev, int m,
                            uint64_t n, uint64_t k, uint64_t capacity,
                            void* ws, size_t ws_bytes, fc_stream_t stream);

/* Exact radix-select path (several reads of g); always succeeds; n_entries == k. */
int fc_topk_encode_exact(const float* g, uint64_t n, uint64_t k, int key_mode, uint64_t seed,
                         uint64_t offset, uint16_t* idx, float* val, uint64_t capacity,
                         uint32_t* cnt, uint64_t* qoff, fc_packet_hdr* hdr, void* ws,
                         size_t ws_bytes, fc_stream_t stream);

/* ---- encode: mask codecs (compression.py:39-60) -------------------------------------
 * codec = FC_CODEC_DROPOUT_* or FC_CODEC_RAND (parity mode: mask from the host's
 * np.random.permutation).  mask_bits (little-endian bit i = element i, N/32 words) is the
 * host-drawn mask in parity mode; NULL selects native Philox Bernoulli(p) keyed by seed.
 * format: FC_FMT_BITMAP (bitmap required) or FC_FMT_IDXVAL (idx required; qoff written when
 * non-NULL). */
int fc_mask_encode(const float* g, uint64_t n, int codec, const uint32_t* mask_bits,
                   double p, uint64_t seed, uint64_t offset, int format, uint16_t* idx,
                   float* val, uint32_t* bitmap, uint64_t capacity, uint32_t* cnt,
                   uint64_t* qoff, fc_packet_hdr* hdr, void* ws, size_t ws_bytes,
                   fc_stream_t stream);

/* ---- decode (compression.py dense result) --------------------------------------------
 * pkt: HOST pointer to one view.  out is float (out_f64 = 0) or double (out_f64 = 1; the
 * reference's float64 dropout result, compression.py:52/60). */
int fc_decode_dense(const fc_packet_view* pkt, int format, uint64_t n, void* out, int out_f64,
                    fc_stream_t stream);

/* ---- FedAVG over packets (aggregation.py:61-63 + gar.py:44), bit-exact fp32 ----------
 * views: DEVICE array of m views (same format), client order = row order of G; FC_FMT_IDXVAL
 * each chunk quarter is folded by its own wave with no barrier, using the views' qoff (a view
 * without qoff is folded by whole-chunk scans).
 * acc[j] = fl(w_0 * d_0[j]);  acc[j] = fl(acc[j] + fl(w_i * d_i[j])) for i = 1..m-1. */
int fc_decode_accumulate(const fc_packet_view* views_dev, int m, int format, uint64_t n,
                         float* acc, fc_stream_t stream);
/* Same fold, continuing the partial sum already held in acc (acc = fl(acc + fl(w_i * d_i))
 * for i = 0..m-1): rows of G split across calls or across GPUs (the exact chained reduce of
 * SURVEY.md §8(e)) give the same bits as one call over all rows.  acc may hold any values: a
 * -0.0 in it (no +0-started sum produces one) follows the dense sum too, staying -0.0 only where
 * every term added to it is -0.0. */
int fc_decode_accumulate_continue(const fc_packet_view* views_dev, int m, int format,
                                  uint64_t n, float* acc, fc_stream_t stream);

/* ---- Gram matrix of a round's packets: G G^T in float64 without the dense G ---------------
 * What a geometry-aware rule needs of the clients (Krum's distances gar.py:184-212,
 * |g_i - g_j|^2 = G_ii + G_jj - 2 G_ij; pc_analysis' singular values aggregation.py:64-67, the
 * square roots of the eigenvalues) computed straight from the packets (fc_gram.hip).
 * views_dev: DEVICE array of m FC_FMT_IDXVAL views with qoff present, as fc_decode_accumulate
 *   takes them; `weight` is ignored.  1 <= m <= FC_GRAM_MAX_M.
 * d_i: the float32 row fc_decode_dense produces for packet i: an entry counts iff its composite
 *   >= T64 (the Philox key for native rand-k; thresh == 0 keeps all; slack entries are listed
 *   but sit below T64 and do not count), dropout-unbiased values are fl32(fl64(v) / p).
 * gram[i*m + j] = sum_t (double)d_i[t] * (double)d_j[t]: every product exact (two float32
 *   multiply exactly in float64), summed in float64.  gram: DEVICE float64[m*m], row-major,
 *   16-B aligned.
 * Non-finite rule: a client whose d_i holds a non-finite element (a kept NaN or +-inf, an
 *   overflowing 1/p scaling, the all-NaN row of dropout-unbiased with p == 0) gets
 *   gram[i][*] = gram[*][i] = NaN, the diagonal included; every other client is unaffected.
 * gram is symmetric bit for bit (one triangle is computed and mirrored).
 * Determinism: the order of summation is a function of the packets, n and m alone (not of the
 *   device, its CU count or timing): the grid and each workgroup's chunk range come from n and
 *   m, partial Grams go to the workspace and a second launch adds them in workgroup order.  No
 *   floating-point atomics, no workgroup waits for another (no fc_fused_order_* handling).  Two
 *   calls on the same packets give the same bits.
 * Stream-ordered; no allocation, no host synchronisation.  ws: fc_gram_workspace_bytes(n, m)
 *   bytes (monotone in n and m), 16-B aligned; it needs NO one-time zeroing: every word the call
 *   reads it has written first.
 * Argument errors return before the GPU is touched: FC_ERR_ARG for a NULL views_dev, gram or
 *   ws, m < 1 or m > FC_GRAM_MAX_M, n == 0 (or n >= 2^32), a gram or ws that is not 16-B
 *   aligned; FC_ERR_WORKSPACE for a short workspace. */
#define FC_GRAM_MAX_M 128
size_t fc_gram_workspace_bytes(uint64_t n, int m);
int fc_packets_gram(const fc_packet_view* views_dev, int m, uint64_t n,
                    double* gram /* DEVICE float64[m*m], row-major, 16-B aligned */,
                    void* ws, size_t ws_bytes, fc_stream_t stream);

/* ---- A round's packets times a dense vector: G v in float64 without the dense G -----------
 * What a rule that is linear in the rows of G needs beside the Gram matrix (aggregate =
 * a v + sum_i c_i d_i with a carried vector v: b = G v and |v|^2; with v = ones the row sums
 * of the reference's explained-variance ratio, spectral_aggregation.py:100-103), computed
 * straight from the packets (fc_dot.hip).
 * views_dev: DEVICE array of m FC_FMT_IDXVAL views with qoff present, as fc_packets_gram takes
 *   them; `weight` is ignored.  1 <= m <= FC_GRAM_MAX_M.
 * d_i: exactly the row fc_packets_gram uses (the same kept-entry rule: composite >= T64, the
 *   Philox key for native rand-k, thresh == 0 keeps all, slack entries do not count;
 *   dropout-unbiased values are fl32(fl64(v) / p)).
 * v: DEVICE float32[n], 16-B aligned, or NULL for the all-ones vector.
 * out: DEVICE float64[m + 1], 16-B aligned.  out[i] = sum_t (double)d_i[t] * (double)v[t] for
 *   i < m (v[t] = 1 when v is NULL: the row sum); out[m] = sum_t (double)v[t]^2 (exactly
 *   (double)n when v is NULL).  Every product is exact, sums are float64 and start from +0.0.
 * Non-finite rule: a client whose d_i holds a non-finite element (a kept NaN or +-inf, an
 *   overflowing 1/p scaling, dropout-unbiased with p == 0) gets out[i] = NaN, the clients the
 *   Gram's rule marks; every other client is unaffected.  If v holds a non-finite element all
 *   m + 1 outputs are NaN.
 * Determinism: the order of summation is a function of the packets, n and m alone: the grid and
 *   each workgroup's chunk range come from n and m, partial sums go to the workspace and a second
 *   launch adds them in a fixed order.  No floating-point atomics, no workgroup waits for
 *   another.  Two calls on the same inputs give the same bits.
 * Stream-ordered; no allocation, no host synchronisation.  ws: fc_dot_workspace_bytes(n, m)
 *   bytes (monotone in n and m), 16-B aligned; it needs NO one-time zeroing.
 * Argument errors return before the GPU is touched: FC_ERR_ARG for a NULL views_dev, out or ws,
 *   m < 1 or m > FC_GRAM_MAX_M, n == 0 (or n >= 2^32), a v, out or ws that is not 16-B aligned;
 *   FC_ERR_WORKSPACE for a short workspace. */
size_t fc_dot_workspace_bytes(uint64_t n, int m);
int fc_packets_dot(const fc_packet_view* views_dev, int m, uint64_t n,
                   const float* v /* DEVICE float32[n], 16-B aligned, or NULL = all ones */,
                   double* out /* DEVICE float64[m + 1], 16-B aligned */,
                   void* ws, size_t ws_bytes, fc_stream_t stream);

/* ---- Coordinate-wise trimmed mean (and median) of a round's packets, without the dense G ----
 * The coordinate-wise robust rules (Yin, Chen, Ramchandran, Bartlett, ICML 2018) computed
 * straight from the packets (fc_trim.hip).
 * views_dev: DEVICE array of m FC_FMT_IDXVAL views with qoff present, as fc_packets_gram takes
 *   them; `weight` is ignored.  1 <= m <= FC_GRAM_MAX_M.
 * d_i: exactly the row fc_packets_gram uses (the same kept-entry rule: composite >= T64, the
 *   Philox key for native rand-k, thresh == 0 keeps all, slack entries do not count;
 *   dropout-unbiased values are fl32(fl64(v) / p)); a coordinate without a kept entry is +0.0.
 * trim: b, the values dropped at each end of a column.  0 <= b, 2 b < m.  b = (m - 1) / 2 is the
 *   coordinate-wise median (the float32 mean of the two middle values for even m).
 * out[t], t < n (DEVICE float32[n], 16-B aligned): the m values d_0[t] .. d_{m-1}[t] in
 *   np.sort's order (-inf first, -0.0 and +0.0 equal, +inf after every finite value, every NaN
 *   after +inf); the b smallest and the b largest dropped; the other m - 2b added in ascending
 *   order from +0.0, every add rounded to float32 (no contraction, no reassociation); the sum
 *   divided by float32(m - 2b) in IEEE float32.  A function of the multiset of a column's values
 *   alone: the order of the clients does not change a bit.  A column of zeros of either sign
 *   gives +0.0.  A NaN is trimmed like a largest value: out[t] is NaN only if more than b values
 *   are NaN or +inf and -inf both survive.  No client is excluded as a whole.
 * One launch, one workgroup per chunk of n.  No floating-point atomics, no workgroup waits for
 *   another (no fc_fused_order_* handling).  Two calls on the same packets give the same bits.
 * Stream-ordered; no allocation, no host synchronisation.  ws: fc_trim_workspace_bytes(n, m)
 *   bytes, 16-B aligned, NO one-time zeroing; the size is 0 today and ws may then be NULL.
 * Argument errors return before the GPU is touched: FC_ERR_ARG for a NULL views_dev or out (or
 *   ws when the size is not 0), m < 1 or m > FC_GRAM_MAX_M, trim < 0, 2 trim >= m, n == 0 (or
 *   n >= 2^32), an out or ws that is not 16-B aligned; FC_ERR_WORKSPACE for a short workspace. */
size_t fc_trim_workspace_bytes(uint64_t n, int m);          /* may be 0 */
int fc_packets_trim(const fc_packet_view* views_dev, int m, uint64_t n, int trim,
                    float* out /* DEVICE float32[n], 16-B aligned */,
                    void* ws, size_t ws_bytes, fc_stream_t stream);

/* ---- The wire form of FC_FMT_IDXVAL packets: pack, unpack, validate (fc_wire.hip) -----------
 * A slotted packet reserves 6n + 12 nch + 96 bytes whatever it keeps.  Its wire form is ONE
 * contiguous byte string that holds the kept entries alone: what a client sends.  Little-endian,
 * every section 16-B aligned, pad bytes zero (openmsftl_amd/csrc/fc_wire_host.h):
 *   0     fc_wire_hdr, 128 bytes: uint32 magic ("FCW1"), uint32 version (1), uint64 total_bytes,
 *         uint64 n_entries (E), uint32 nch, uint32 status, fc_packet_hdr pkt
 *   128   uint64 qoff[nch]   the slotted word format over the KEPT entries (quarter 1/2/3 starts
 *                            in bits 0-15 / 16-31 / 32-47, cnt in bits 48-63)
 *         uint32 start[nch]  exclusive prefix sum of the counts
 *         uint16 idx[E]      chunk-local, ascending inside each chunk
 *         float  val[E]      the stored values bit for bit (the decoders apply 1/p from pkt.p)
 * Kept: exactly the entries fc_packets_gram counts (composite >= T64, the Philox key for native
 *   rand-k, thresh == 0 keeps every listed entry; the quarter an entry is listed under matches
 *   its index).  A resolved top-k / native rand-k packet has E == k.
 * pkt is canonical: the source header's thresh, n, k, index_bits, codec, seed, offset, p, chunk,
 *   format, key_mode; lower = thresh, n_entries = E (also for mask packets), status = 0,
 *   n_definite = n_cand = reserved = 0.  The bytes are a function of the kept content and those
 *   fields alone: a sampled-bracket encode and fc_topk_encode_exact of one gradient pack alike.
 * fc_wire_bytes(n, E): HOST, the exact size; monotone in E (0 for n == 0 or n, E >= 2^32).
 *
 * fc_wire_pack_batch: m packets (views_dev: DEVICE array of m FC_FMT_IDXVAL views with qoff, as
 *   fc_packets_gram takes them; `weight` ignored) into m wire buffers (jobs_dev: DEVICE array of
 *   m fc_wire_job: a 16-B aligned DEVICE buffer of at least 128 bytes and its capacity in bytes).
 *   A source header whose status is not OK: that status goes into the wire `status` and nothing
 *   else is promised.  A capacity below the packet's size: status FC_STATUS_OVERFLOW, the
 *   128-byte header alone (total_bytes = the size needed, n_entries = E) and nothing past the
 *   capacity.  Otherwise exactly total_bytes bytes are written.  Launches: count, scan, compact
 *   (grid.y = the client; grids from n and m alone; no workgroup waits for another; no atomics):
 *   two calls give the same bytes.  Stream-ordered, no allocation, no host synchronisation.
 *   ws: fc_wire_workspace_bytes(n, m) bytes (monotone in n and m), 16-B aligned, needs NO zeroing.
 * fc_wire_unpack_batch: m wire packets on the device (jobs_dev: buffer and its byte length, as
 *   the HOST knows it) into m slotted packets (views_dev: the DESTINATION packets, written
 *   through: idx, val, cnt, qoff, hdr all present, capacity fc_packet_capacity(n)).  Writes the
 *   listed slot positions, cnt, qoff and hdr (= pkt) only: never the 6n capacity.  Memory safe
 *   whatever the bytes hold: every read is below the byte length, start and cnt are clamped
 *   against E and the section ends, every write lands in its chunk's slot; a buffer whose header
 *   does not fit n or the length becomes an empty packet with status FC_STATUS_OVERFLOW.  The
 *   index VALUES are not checked here (consumers use them as LDS locations): bytes that come
 *   from outside pass fc_wire_validate first.
 * Both: 1 <= m <= 65535, 1 <= n < 2^32, NULL tables: FC_ERR_ARG; a short workspace:
 *   FC_ERR_WORKSPACE; all before the GPU is touched.
 * fc_wire_validate: HOST bytes, no GPU.  FC_OK, or FC_ERR_ARG with the reason in
 *   fc_last_error().  In this order, reading nothing past len: (1) len >= 128, magic, version,
 *   total_bytes == len; (2) pkt: 1 <= n < 2^32, n == n_expected unless that is 0, k <= n,
 *   index_bits, chunk, format IDXVAL, codec 1..4, key_mode 0..1, both statuses 0; (3) nch and
 *   total_bytes == fc_wire_bytes(n, E); (4) per chunk q1 <= q2 <= q3 <= cnt <= 8192, start the
 *   prefix sum, the counts summing to E == pkt.n_entries; (5) per quarter range strictly
 *   ascending indices of that quarter with c * 8192 + idx < n; (6) zero pads.  It does not check
 *   entries against thresh: a listed entry below it is dropped by every decoder.
 * fc_wire_fold (fc_wire_fold.hip): the FedAVG of m wire packets on the device without unpacking
 *   them.  jobs_dev: DEVICE array of m {wire buffer, byte length as the HOST knows it}, as
 *   fc_wire_unpack_batch takes it; weights_dev: DEVICE fp32[m]; acc: n floats, 16-B aligned,
 *   started from +0 or, with continue_sum != 0, continued.  For every buffer, whatever its bytes
 *   hold, acc gets the bits that fc_wire_unpack_batch into fresh packets followed by
 *   fc_decode_accumulate (fc_decode_accumulate_continue) with the same weights would give: the
 *   decoders' keep rule per entry (a listed entry below thresh is dropped), 1/p for
 *   dropout-unbiased, NaN for the coordinates a p == 0 packet does not keep, a buffer whose header
 *   does not fit n or the length a packet with no entries.  Memory safe whatever the bytes hold:
 *   the header is read only when the length is >= 128; both tables and the entries are read only
 *   when fc_wire_bytes(n, E) <= the length; start and the quarter offsets are clamped against E
 *   and each other as the unpack clamps them, so every read is below the byte length; every LDS
 *   location is masked into or compared against its 2048-element quarter.  As for the unpack,
 *   the index VALUES are not checked: bytes from outside pass fc_wire_validate first.
 *   1 <= m <= 65535: launches of at most 128 packets, each continuing the same left-to-right
 *   sum, so the result does not depend on how a round is cut into calls.  One workgroup per
 *   chunk, no workgroup waits for another, no atomics on acc: two calls give the same bits.
 *   Stream-ordered, no allocation, no workspace, no host synchronisation.  NULL tables or acc,
 *   m or n out of range, a misaligned acc: FC_ERR_ARG before the GPU is touched. */
typedef struct fc_wire_job {
  void* wire;            /* DEVICE wire buffer, 16-B aligned                       */
  uint64_t bytes;        /* pack: its capacity; unpack: the packet's byte length    */
} fc_wire_job;           /* 16 bytes */
uint64_t fc_wire_bytes(uint64_t n, uint64_t n_entries);
size_t fc_wire_workspace_bytes(uint64_t n, int m);
int fc_wire_pack_batch(const fc_packet_view* views_dev, const fc_wire_job* jobs_dev, int m,
                       uint64_t n, void* ws, size_t ws_bytes, fc_stream_t stream);
int fc_wire_unpack_batch(const fc_wire_job* jobs_dev, const fc_packet_view* views_dev, int m,
                         uint64_t n, fc_stream_t stream);
int fc_wire_validate(const void* host_bytes, size_t len, uint64_t n_expected /* 0 = any */);
int fc_wire_fold(const fc_wire_job* jobs_dev, const float* weights_dev, int m, uint64_t n,
                 float* acc, int continue_sum, fc_stream_t stream);

/* ---- FedAVG over dense rows (gar.py:44 for 'full'): rows = DEVICE array of m row
 * pointers, w = DEVICE fp32[m]. */
int fc_weighted_sum_dense(const float* const* rows, const float* w, int m, uint64_t n,
                          float* out, fc_stream_t stream);
/* Same sum continuing the partial sum already in out (out = fl(out + fl(w_i * row_i)) for
 * i = 0..m-1): 'full' rows streamed group by group from host memory (aggregation.py:61-63)
 * fold to the same bits as one call over all rows. */
int fc_weighted_sum_dense_continue(const float* const* rows, const float* w, int m, uint64_t n,
                                   float* out, fc_stream_t stream);

/* ---- flat-layout staging on the device (model_helper.py:11-35, client.py:44,52-53) ------
 * params_dev: DEVICE array of `count` fp32 parameter pointers; offsets_dev: DEVICE
 * uint64[count + 1] prefix offsets into the flat vector (max_size = largest parameter).
 * scatter = 0: flat[off_p + i] <- param_p[i]; with grad != NULL first
 *   grad = fl32(flat_old - param)  (client.py:53: current_weights - updated_model_weights),
 *   i.e. flatten_params + the client delta in one pass, flat keeping the new weights;
 * scatter = 1: param_p[i] <- flat[off_p + i]  (dist_weights_to_model / dist_grads_to_model). */
int fc_flat_stage(const float* const* params_dev, const uint64_t* offsets_dev, int count,
                  uint64_t max_size, float* flat, float* grad, int scatter, fc_stream_t stream);

/* ---- hierarchical merge (aggregation.py:80-93): a cluster's mean
 * np.mean(G[s:e, :], axis=0) is the +0-started row-order sum (fc_decode_accumulate /
 * fc_weighted_sum_dense with weights 1.0) divided once by the row count: x = fl(x / d), in
 * place, x a DEVICE fp32[n] (16-B aligned). */
int fc_div_scalar(float* x, uint64_t n, float d, fc_stream_t stream);

/* ---- QSGD quantiser (compression.py:62-74, the reference's commented formula; opt-in,
 * parity unpinned with respect to the reference, pinned to oracle/qsgd_oracle.py) ------
 * q_i = sign(g_i) * ||g|| / (s tau) * floor(s |g_i| / ||g|| + U_i), s = 2^bits (1..14),
 * tau = 1 + min(sqrt(n)/s, n/s^2), U_i from Philox(seed, offset).  Codes: W = 4/8/16-bit
 * (sign | level) packed little-endian into code_words >= fc_qsgd_code_words(n, bits) uint32
 * (16-B aligned).  The header records ||g|| (double, field p), bits (field k), the Philox
 * key/counter, codec FC_CODEC_QSGD and format FC_FMT_QSGD.  ws: fc_qsgd_workspace_bytes(),
 * zeroed once.  Decoders take fc_packet_view with idx = codes. */
uint64_t fc_qsgd_code_words(uint64_t n, int bits);
size_t fc_qsgd_workspace_bytes(void);
int fc_qsgd_encode(const float* g, uint64_t n, int bits, uint64_t seed, uint64_t offset,
                   uint32_t* codes, uint64_t code_words, fc_packet_hdr* hdr, void* ws,
                   size_t ws_bytes, fc_stream_t stream);
int fc_qsgd_decode(const fc_packet_view* pkt, uint64_t n, float* out, fc_stream_t stream);
/* FedAVG over QSGD packets (views_dev: DEVICE array of m views, weights in the views):
 * out = fl(... fl(+0 + fl(w_0 q_0)) ...) in row order (gar.py:44); continue_sum != 0 folds
 * into the partial sum already in out. */
int fc_qsgd_decode_accumulate(const fc_packet_view* views_dev, int m, uint64_t n, float* out,
                              int continue_sum, fc_stream_t stream);

/* ---- QSGD with error feedback and the QSGD packet's wire form (fc_qsgd.hip, fc_qsgd_host.h) ----
 * The quantiser above divides by tau, so E[q] = g / tau: a contraction, the form EF-signSGD
 * (Karimireddy, Rebjock, Stich, Jaggi, ICML 2019) takes error feedback for.  For a float32 gradient
 * g[n], n >= 1, and an optional float32 residual e[n]:
 *   a[t] = fl32(g[t] + e[t]), one IEEE add (so -0.0 + +0.0 = +0.0); a[t] = g[t] without res_in
 *   header (all 96 bytes) and codes: byte for byte what fc_qsgd_encode writes for an array holding
 *          a: the fp64 norm summed in the same fixed order (same grid, same per-thread order, same
 *          tail), the same Philox map, the same choice between the fp32 and the fp64 form of the
 *          level, the clamp to s and NaN -> level 0.  Nothing is special-cased
 *   q[t] = what fc_qsgd_decode writes for that packet: (float)(+-(norm / (s tau)) * l), an fp64
 *          product and one rounding
 *   e'[t] = fl32(a[t] - q[t]), one IEEE subtract, into res_out (a non-finite gradient poisons it
 *          exactly as this arithmetic says)
 * fc_qsgd_encode_ef: g, res_in (NULL: none), res_out (NULL: not wanted) and codes all 16-B aligned;
 *   res_out may not overlap g or res_in; code_words >= fc_qsgd_code_words(n, bits).  With both
 *   residual pointers NULL the call is fc_qsgd_encode.  Two launches (the norm pass, whose last
 *   arriver writes the header, and the quantise pass), neither waits in-kernel for another
 *   workgroup: no fc_fused_order_* handling.  ws: fc_qsgd_workspace_bytes(), fc_qsgd_encode's
 *   contract.  Bytes with both residuals: 16N read in two passes over g and e, 4N + N W / 8 written.
 *   Argument errors (NULL, n, bits, alignment, overlap, code_words: FC_ERR_ARG; a short workspace:
 *   FC_ERR_WORKSPACE) are reported before the GPU is touched.
 * Wire form (openmsftl_amd/csrc/fc_qsgd_host.h): a 128-byte header (uint32 magic "FCQ1", uint32
 *   version 1, uint64 total_bytes, 16 zero bytes, the canonical fc_packet_hdr) and the
 *   fc_qsgd_code_words(n, bits) uint32 of codes padded with zero words to a multiple of 4.
 *   fc_qsgd_wire_bytes: its size, a function of n and bits alone; 0 for bits outside [1, 14].
 * fc_qsgd_wire_validate: HOST bytes, no GPU.  FC_OK, or FC_ERR_ARG with the reason in
 *   fc_last_error(), reading nothing past len: NULL; shorter than the header; a wrong magic or
 *   version; total_bytes != len; the reserved bytes; n = 0 or n != n_expected (unless that is 0);
 *   codec or format other than QSGD; k (bits) outside [1, 14]; n_entries != n; a status other than
 *   OK; key_mode other than FC_KEY_PHILOX; a field that must be zero (thresh, lower, index_bits,
 *   n_definite, n_cand, chunk, reserved); a negative norm p (NaN excepted; p is any other double);
 *   len != fc_qsgd_wire_bytes(n, bits); a code whose level exceeds s = 2^bits (the field is W - 1
 *   bits wide; the encoder never writes one); a non-zero code at or past n inside the last group;
 *   a non-zero pad word.  seed and offset may be anything.  fc_wire_validate and
 *   fc_sign_wire_validate reject these bytes by their magic. */
int fc_qsgd_encode_ef(const float* g, const float* res_in /* NULL: none */,
                      float* res_out /* NULL: not wanted */, uint64_t n, int bits,
                      uint64_t seed, uint64_t offset, uint32_t* codes, uint64_t code_words,
                      fc_packet_hdr* hdr, void* ws, size_t ws_bytes, fc_stream_t stream);
uint64_t fc_qsgd_wire_bytes(uint64_t n, int bits);
int fc_qsgd_wire_validate(const void* host_bytes, size_t len, uint64_t n_expected /* 0 = any */);

/* ---- scaled sign with error feedback, its FedAVG fold and the majority vote (fc_sign.hip) ----
 * The 1-bit codec (EF-signSGD: Karimireddy, Rebjock, Stich, Jaggi, ICML 2019; opt-in, no reference
 * counterpart) and the cheapest coordinate-wise robust rule over its packets (signSGD with
 * majority vote: Bernstein, Zhao, Azizzadenesheli, Anandkumar, ICLR 2019).  For a float32
 * gradient g[n], n >= 1, and an optional float32 residual e[n]:
 *   a[t] = fl32(g[t] + e[t]), one IEEE add (so -0.0 + +0.0 = +0.0); a[t] = g[t] without a residual
 *   s    = fl32(S / (double)n), S = sum_t (double)|a[t]| in float64, in an order fixed by n alone
 *          (no floating-point atomics: two calls give the same bits); non-finite elements make s
 *          inf or NaN by plain IEEE arithmetic, nothing is special-cased
 *   b[t] = the IEEE sign bit of a[t] (-0.0 is negative, a NaN goes by its sign bit; the sign of a
 *          NaN that the add itself produces, inf + -inf, is the hardware's), little-endian: bit
 *          t % 32 of uint32 word[t / 32], the convention of mask_bits.  fc_sign_words(n) words:
 *          ceil(n / 32) rounded up to a multiple of 4; bits at and past n and the pad words are
 *          written as zero
 *   q[t] = b[t] ? -s : +s                       (fc_sign_decode)
 *   e'[t] = fl32(a[t] - q[t]), one IEEE subtract (res_out; a non-finite gradient poisons it exactly
 *          as this arithmetic says)
 *   header: codec FC_CODEC_SIGN, format FC_FMT_SIGN, n, k = n_entries = n, status FC_STATUS_OK,
 *          p = (double)s, every other field zero.  A view carries the words in `bitmap`; idx, val,
 *          cnt and qoff are NULL.
 * fc_sign_encode: g, res_in (NULL: none), res_out (NULL: not wanted), words all 16-B aligned;
 *   res_out may not overlap g or res_in (the rule of fc_topk_encode_ef); n_words >=
 *   fc_sign_words(n).  Two launches (the norm pass, whose last arriver writes the header, and the
 *   streaming pass), neither waits in-kernel for another workgroup: no fc_fused_order_* handling.
 *   ws: fc_sign_workspace_bytes(n) bytes, 8-B aligned, zeroed once (self-cleaning afterwards), one
 *   per stream.  Bytes: 8N (16N with a residual) read, N/8 (+ 4N) written.
 * fc_sign_decode: pkt a HOST pointer to one view; out float32[n], 16-B aligned.
 * fc_sign_fold: the FedAVG of m packets (views_dev: DEVICE array of m views, the weights in the
 *   views, 1 <= m <= 65535) with the bits of fc_weighted_sum_dense on the m decoded rows: per
 *   coordinate the terms +-c_i, c_i = fl32(w_i * s_i), added in row order from +0.0
 *   (continue_sum != 0: from the sum already in out, as fc_decode_accumulate_continue; a round
 *   cut into groups gives the bits of one call).  Bytes: m N/8 + 4N (+ 4N when continuing).
 * fc_sign_vote: neg = #{i : b_i[t]}; out[t] = -eta if 2 neg > m, +eta if 2 neg < m, +0.0 on a tie.
 *   Integer counting: any client order gives the same result; weights and scales play no part.
 * Both: one launch, no workgroup waits for another, no atomics, stream-ordered, no allocation, no
 *   workspace; out float32[n], 16-B aligned; every view's words 16-B aligned (the caller's
 *   contract: the table is device memory).
 * fc_sign_wire_validate: HOST bytes, no GPU (openmsftl_amd/csrc/fc_sign_host.h).  The wire form is
 *   a 128-byte header (uint32 magic "FCS1", uint32 version 1, uint64 total_bytes, 16 zero bytes,
 *   the canonical fc_packet_hdr above) and 4 fc_sign_words(n) bytes of words: a function of n
 *   alone.  FC_OK, or FC_ERR_ARG with the reason in fc_last_error(), reading nothing past len:
 *   a wrong length, magic or version; n = 0 or n != n_expected (unless that is 0); codec or format
 *   other than sign; k or n_entries != n; a status other than OK; a field that must be zero; a
 *   negative p (NaN excepted); a p that is not exactly a float32 value; a set bit at or past n; a
 *   non-zero pad word.  fc_wire_validate rejects these bytes by their magic.
 * fc_sign_fold_form (measurement, not thread-safe): how the following fc_sign_fold / fc_sign_vote
 *   launches bring the words to the waves: 0 scalar loads and 1 vector loads with v_readlane
 *   (the 64-bit word wave-uniform, used as a lane mask), 2 one word per lane (the default: the
 *   fastest measured), -1 the default.  The results do not depend on it.
 * fc_sign_encode_batch: fc_sign_encode for m clients of one length n, 1 <= m <= 65535.  Client c's
 *   header (all 96 bytes), its fc_sign_words(n) words (tail bits and pad words zero) and its
 *   res_out are, byte for byte, what fc_sign_encode writes for jobs[c]'s pointers.  jobs_dev is a
 *   DEVICE array (8-B aligned), so the library cannot look inside it: has_res_in / has_res_out say
 *   what the WHOLE batch carries (a job's res_in / res_out is then non-NULL in every job, else
 *   ignored); 16-B alignment of every g / res_in / res_out / words, their length, that a job's
 *   res_out overlaps no g / res_in / res_out of the batch, and that words and headers are distinct
 *   per job, are the caller's contract.  Without res_out ONE launch for all m clients: the norm
 *   pass's grid and loop per client (client = blockIdx.y), which also ballots and stores the words
 *   of every 256 elements it reads, so g (and res_in) are read once: 4N (8N) + N/8 bytes per
 *   client.  With res_out a second launch for all m streams e', each client's s read from its own
 *   header.  No workgroup waits for another; stream-ordered, no allocation, no host
 *   synchronisation.  ws: fc_sign_batch_workspace_bytes(n, m) bytes (m lone workspaces; monotone
 *   in m), 8-B aligned, zeroed once (self-cleaning afterwards), one per stream.
 * Argument errors (NULL, n, m, alignment, overlap, n_words: FC_ERR_ARG; a short workspace:
 *   FC_ERR_WORKSPACE) are reported before the GPU is touched. */
typedef struct fc_sign_job {
  const float*   g;        /* gradient, n floats, 16-B aligned                                  */
  const float*   res_in;   /* residual e, or NULL (then NULL for every job of the batch)        */
  float*         res_out;  /* new residual e', or NULL (then NULL for every job of the batch)   */
  uint32_t*      words;    /* >= fc_sign_words(n) uint32, 16-B aligned                          */
  fc_packet_hdr* hdr;
  uint64_t       reserved; /* 0 */
} fc_sign_job;             /* 48 bytes */
uint64_t fc_sign_words(uint64_t n);
size_t fc_sign_workspace_bytes(uint64_t n);
int fc_sign_encode(const float* g, const float* res_in /* NULL: none */,
                   float* res_out /* NULL: not wanted */, uint64_t n, uint32_t* words,
                   uint64_t n_words, fc_packet_hdr* hdr, void* ws, size_t ws_bytes,
                   fc_stream_t stream);
size_t fc_sign_batch_workspace_bytes(uint64_t n, int m);
int fc_sign_encode_batch(const fc_sign_job* jobs_dev, int m, uint64_t n, int has_res_in,
                         int has_res_out, void* ws, size_t ws_bytes, fc_stream_t stream);
int fc_sign_decode(const fc_packet_view* pkt, uint64_t n, float* out, fc_stream_t stream);
int fc_sign_fold(const fc_packet_view* views_dev, int m, uint64_t n, float* out, int continue_sum,
                 fc_stream_t stream);
int fc_sign_vote(const fc_packet_view* views_dev, int m, uint64_t n, float eta, float* out,
                 fc_stream_t stream);
int fc_sign_wire_validate(const void* host_bytes, size_t len, uint64_t n_expected /* 0 = any */);
int fc_sign_fold_form(int form);

/* ---- The clients' geometry from scaled-sign packets: Gram matrix and G v (fc_sign_gram.hip) ----
 * What fc_packets_gram and fc_packets_dot give for idx/val packets, for a round of sign packets,
 * so that Krum, the linear rules and pc_analysis "gram" can take 1-bit clients.  With
 * d_i[t] = b_i[t] ? -s_i : +s_i (the row fc_sign_decode makes):
 *   <d_i, d_j> = s_i s_j (n - 2 H_ij),  H_ij = popcount(words_i XOR words_j)
 *   <d_i, v>   = s_i D_i,               D_i  = sum_t (b_i[t] ? -v[t] : +v[t])
 * views_dev: DEVICE array of m FC_FMT_SIGN views, as fc_sign_fold takes them: the words in
 *   `bitmap`, 16-B aligned, with zero bits at and past n and zero pad words (the encoder's and the
 *   validator's guarantee); s_i is the float32 scale in the packet header's p; `weight` is ignored.
 *   1 <= m <= FC_GRAM_MAX_M, 1 <= n < 2^32.
 * fc_sign_gram: H_ij is the exact integer count of differing bits among the first n.
 *   gram[i*m + j] = fl64((fl64(s_i) * fl64(s_j)) * (double)(n - 2 H_ij)): the first product is
 *   exact (48 significant bits), the integer is exact (below 2^32 in magnitude), so the entry is
 *   ONE IEEE float64 multiply: the correctly rounded value of the true inner product of the decoded
 *   rows, whatever the order of anything.  The diagonal is s_i^2 n (H_ii = 0).  gram: DEVICE
 *   float64[m*m], row-major, 16-B aligned; symmetric bit for bit (one triangle is computed and
 *   mirrored); two calls, or any permutation of workgroups, give the same bits.
 *   Non-finite rule: a client whose s_i is NaN or +-inf gets gram[i][*] = gram[*][i] = NaN, the
 *   diagonal included (the rule of fc_packets_gram); every other client is unaffected.  s_i == 0
 *   follows plain IEEE: zeros of either sign.
 * fc_sign_dot: out[i] = fl64(s_i) * D_i for i < m, D_i summed in float64 from +0.0 over
 *   (b_i[t] ? -(double)v[t] : +(double)v[t]); with v == NULL (the all-ones vector) D_i =
 *   (double)(n - 2 popcount_i) exactly.  out[m] = sum_t (double)v[t]^2 (exactly (double)n when v
 *   is NULL), as fc_packets_dot defines it.  v: DEVICE float32[n], 16-B aligned, or NULL; out:
 *   DEVICE float64[m + 1], 16-B aligned.
 *   Non-finite rule: a non-finite s_i gives out[i] = NaN; a non-finite element in v makes all
 *   m + 1 outputs NaN.
 *   Determinism: the order of summation is a function of n and m alone: the grid and each
 *   workgroup's range of words come from them, every thread adds its coordinates in index order,
 *   the partial sums go to the workspace and a second launch adds them in index order.
 * Both: stream-ordered; no allocation, no host synchronisation; no floating-point atomics; no
 *   workgroup waits in-kernel for another (no fc_fused_order_* handling).  The Gram's integer
 *   counts are added inside a workgroup with integer LDS atomics (any order, the same integers)
 *   and across workgroups by a finishing launch.  ws: fc_sign_gram_workspace_bytes(n, m) /
 *   fc_sign_dot_workspace_bytes(n, m) bytes (monotone in n and m), 16-B aligned, NO one-time
 *   zeroing: every word a call reads it has written first.
 * Argument errors return before the GPU is touched: FC_ERR_ARG for a NULL views_dev, gram / out or
 *   ws, m < 1 or m > FC_GRAM_MAX_M, n == 0 (or n >= 2^32), a gram, v, out or ws that is not 16-B
 *   aligned; FC_ERR_WORKSPACE for a short workspace. */
size_t fc_sign_gram_workspace_bytes(uint64_t n, int m);
int fc_sign_gram(const fc_packet_view* views_dev, int m, uint64_t n,
                 double* gram /* DEVICE float64[m*m], row-major, 16-B aligned */,
                 void* ws, size_t ws_bytes, fc_stream_t stream);
size_t fc_sign_dot_workspace_bytes(uint64_t n, int m);
int fc_sign_dot(const fc_packet_view* views_dev, int m, uint64_t n,
                const float* v /* DEVICE float32[n], 16-B aligned, or NULL = all ones */,
                double* out /* DEVICE float64[m + 1], 16-B aligned */,
                void* ws, size_t ws_bytes, fc_stream_t stream);

/* ---- Coordinate-wise trimmed mean (and median) of scaled-sign packets (fc_sign_trim.hip) ----
 * What fc_packets_trim gives for idx/val packets, for a round of sign packets: the coordinate-wise
 * robust rules (Yin, Chen, Ramchandran, Bartlett, ICML 2018) for 1-bit clients, without one decoded
 * row.  A column holds only the values -+s_i, so np.sort's order of it follows from the order of
 * the m scales: nothing is sorted per coordinate.
 * views_dev: DEVICE array of m FC_FMT_SIGN views, exactly as fc_sign_gram takes them: the words in
 *   `bitmap`, 16-B aligned, with zero bits at and past n and zero pad words; s_i is the float32
 *   scale in the packet header's p; `weight` is ignored.  1 <= m <= FC_GRAM_MAX_M, 1 <= n < 2^32.
 * trim: b, the values dropped at each end of a column.  0 <= b, 2 b < m.  b = (m - 1) / 2 is the
 *   coordinate-wise median (the float32 mean of the two middle values for even m).
 * out[t], t < n (DEVICE float32[n], 16-B aligned): fc_packets_trim's definition applied to the
 *   column d_i[t] = b_i[t] ? -s_i : +s_i (the row fc_sign_decode makes): the m values in np.sort's
 *   order (-0.0 and +0.0 equal, +inf after every finite value, every NaN of either sign after
 *   +inf); the b smallest and the b largest dropped; the other m - 2b added in ascending order
 *   from +0.0, every add rounded to float32 (no contraction, no reassociation); the sum divided
 *   once by float32(m - 2b) in IEEE float32.  A function of the multiset of a column's values
 *   alone: any order of the clients and any two calls give the same bits.  A client with a NaN
 *   scale contributes a NaN at the top end of every column and is trimmed like a largest value:
 *   out[t] is NaN only if more than b scales are NaN (or +inf and -inf both survive).  No client
 *   is excluded as a whole.  With every scale equal to eta the median is fc_sign_vote(eta) bit for
 *   bit (2 eta finite), a tie giving +0.0.  The encoder and the validator make s_i >= 0 or NaN;
 *   a scale with the sign bit set is taken as it stands (the client of |s_i| with every bit
 *   flipped).
 * One launch, the grid a function of n alone.  The scales are ranked on the device from the
 *   headers, once per workgroup (the host reads no header); a lane owns 32 consecutive coordinates
 *   and walks the clients' bits in rank order, twice; the b steps at each end that cannot land
 *   in the window [b, m - b) only count or are skipped.  No floating-point atomics, no workgroup
 *   waits for another (no fc_fused_order_* handling).
 * Stream-ordered; no allocation, no host synchronisation.  ws: fc_sign_trim_workspace_bytes(n, m)
 *   bytes, 16-B aligned, NO one-time zeroing; the size is 0 today and ws may then be NULL.
 * Argument errors return before the GPU is touched: FC_ERR_ARG for a NULL views_dev or out (or
 *   ws when the size is not 0), m < 1 or m > FC_GRAM_MAX_M, trim < 0, 2 trim >= m, n == 0 (or
 *   n >= 2^32), an out or ws that is not 16-B aligned; FC_ERR_WORKSPACE for a short workspace. */
size_t fc_sign_trim_workspace_bytes(uint64_t n, int m);     /* may be 0 */
int fc_sign_trim(const fc_packet_view* views_dev, int m, uint64_t n, int trim,
                 float* out /* DEVICE float32[n], 16-B aligned */,
                 void* ws, size_t ws_bytes, fc_stream_t stream);

/* ---- float64 gradients ------------------------------------------------------------
 * The reference reaches the codec with float64 gradients after RandomGaussian with
 * noise_scale == 0 (attack_models.py:105-106); G takes that dtype (aggregation.py:61) and
 * every codec and gar.py:44 then compute in float64.  These entry points produce the dense
 * float64 result compress() returns (all buffers DEVICE, float64, 8-B aligned).
 * fc_topk_dense_f64: 'top' (key_mode MAGNITUDE) / native 'rand' (PHILOX), exact radix select
 *   of the k-th largest (key64 << 32 | idx) (<= 8 passes over g) then q = selected ? g : +0;
 *   same tie rule as the fp32 path.  ws: fc_workspace_bytes(n), zeroed once.
 * fc_mask_dense_f64: codec RAND (mask_bits required: q = keep ? g : +0), DROPOUT_BIASED
 *   (q = g * keep) or DROPOUT_UNBIASED (q = (g * keep) / p), the reference's float64
 *   arithmetic including -0 and NaN (inf * 0); mask_bits NULL = native Philox Bernoulli(p).
 * fc_mask_dense_f32: the same on a float32 gradient (4-B aligned), promoted exactly: the
 *   float64 array compression.py:47-60 returns for float32 client.grad, -0.0 included
 *   (replaces compression.py:51-53 / :58-60 on the drop-in path).
 * fc_weighted_sum_dense_f64: gar.py:44 when G or the weights are float64: rows = DEVICE
 *   array of m row pointers (float32 if rows_f64 == 0, promoted exactly), w = DEVICE
 *   float64[m]; out = +0-started row-order fp64 sum of fl64(g_i * w_i); continue_sum != 0
 *   continues the sum already in out.
 * fc_div_scalar_f64: x = fl64(x / d) in place (np.mean's count division for float64 G).
 * fc_topk_dense_f64_sampled: 'top' (magnitude keys, 0 < k < n, g / out 16-B aligned) by the
 *   fp32 design on each double's high 31-bit key: sampled bracket, ONE streaming pass that
 *   writes out and lists the bracket's candidates, exact select among them, slack fix-up
 *   (replaces compression.py:31-37 for float64 client.grad; 8N read + 8N written instead of
 *   <= 8 passes of 8N).  Writes *status (DEVICE uint32) = FC_STATUS_OK, or
 *   FC_STATUS_RETRY_EXACT when the bracket missed (or > 2048 candidates share the rank's
 *   histogram bin): out is then not valid and the caller runs fc_topk_dense_f64 (exact).  Same result bits as
 *   fc_topk_dense_f64.  ws: fc_workspace_bytes(n), zeroed once. */
int fc_topk_dense_f64_sampled(const double* g, uint64_t n, uint64_t k, double* out, void* ws,
                              size_t ws_bytes, uint32_t* status, fc_stream_t stream);
int fc_topk_dense_f64(const double* g, uint64_t n, uint64_t k, int key_mode, uint64_t seed,
                      uint64_t offset, double* out, void* ws, size_t ws_bytes,
                      fc_stream_t stream);
int fc_mask_dense_f64(const double* g, uint64_t n, int codec, const uint32_t* mask_bits, double p,
                      uint64_t seed, uint64_t offset, double* out, fc_stream_t stream);
int fc_mask_dense_f32(const float* g, uint64_t n, int codec, const uint32_t* mask_bits, double p,
                      uint64_t seed, uint64_t offset, double* out, fc_stream_t stream);
int fc_weighted_sum_dense_f64(const void* const* rows, int rows_f64, const double* w, int m,
                              uint64_t n, double* out, int continue_sum, fc_stream_t stream);
int fc_div_scalar_f64(double* x, uint64_t n, double d, fc_stream_t stream);

/* ---- NumPy's legacy MT19937 stream on the device: the reference's own dropout draws ---------
 * Replaces np.random.binomial(1, p, (n,)) of compression.py:51 / :58 (the process-global legacy
 * RandomState; NumPy's random_binomial_inversion for n = 1: U = random_sample() from two
 * 32-bit outputs, kept iff U > exp(log(1 - p)), complemented for p > 0.5).  A round draws the
 * masks of `rows` consecutive dropout rows of length n, row r starting 2 r n outputs after the
 * state (key, pos) of np.random.get_state(); the mask words equal
 * bitmask_words(np.random.binomial(1, p, (n,)), n, True) bit for bit, and the state block
 * holds the state np.random would be left in (openmsftl_amd/csrc/fc_mt.hip; pinned against
 * NumPy in tests/test_mt19937.py).
 *   fc_mt_plan: the jump polynomials of length n for up to `rows` rows (computed on the host,
 *     cached per n; the first n costs ~0.1-0.5 s) copied into the DEVICE buffer `plan`
 *     (fc_mt_plan_bytes); synchronises `stream`.  Reusable for every round of length n and
 *     at most `rows` rows.
 *   fc_mt_begin: the round's starting state (key: HOST uint32[624], pos in [0, 624]) into
 *     the DEVICE workspace (fc_mt_workspace_bytes(rows), 256-B aligned), each row's window
 *     and raw sequence, and the state after `rows` rows into the fc_mt_state at ws offset 0.
 *   fc_mt_binomial: row `row`'s mask (mask_bits: DEVICE uint32[ceil(n/32)], bits >= n zero),
 *     after fc_mt_begin on the same stream.  p outside [0, 1] is FC_ERR_ARG (NumPy raises
 *     ValueError).  NumPy's rare redraw (U - qn > p qn / (1 - p) after U > qn, ~2^-52 per
 *     element) is not reproduced: fc_mt_state.redraw becomes non-zero and the caller must draw
 *     the round on the host instead.
 *   fc_mt_jump_poly / fc_mt_charpoly (HOST, no GPU): z^d mod chi and chi (MT19937's
 *     characteristic polynomial, degree 19937) as 624 little-endian words (bit i = z^i). */
#define FC_MT_SEG 32768           /* mask elements per generator wave */
typedef struct {
  uint32_t key[624];              /* np.random.get_state()[1] after the round */
  uint32_t pos;                   /* ... [2] */
  uint32_t redraw;                /* != 0: NumPy would have redrawn: use host draws */
  uint32_t rows;
  uint32_t start_pos;
} fc_mt_state;
size_t fc_mt_plan_bytes(uint64_t n, int rows);
size_t fc_mt_workspace_bytes(int rows);
int fc_mt_plan(uint64_t n, int rows, void* plan, size_t plan_bytes, fc_stream_t stream);
int fc_mt_begin(const void* plan, size_t plan_bytes, uint64_t n, int rows, const uint32_t* key,
                uint32_t pos, void* ws, size_t ws_bytes, fc_stream_t stream);
int fc_mt_binomial(const void* plan, size_t plan_bytes, uint64_t n, int rows, int row, double p,
                   uint32_t* mask_bits, void* ws, size_t ws_bytes, fc_stream_t stream);
int fc_mt_jump_poly(uint64_t d, uint32_t* out_words);
int fc_mt_charpoly(uint32_t* out_words);

/* ---- np.random.permutation(n)[:k] on the device: the reference's own 'rand' draws ------------
 * Replaces np.random.permutation(n)[:k] of compression.py:43 on the process-global legacy
 * RandomState (NumPy's shuffle of arange(n): for i = n-1 .. 1, j = random_interval(i) by masked
 * rejection of 32-bit MT19937 outputs, swap x[i], x[j]).  idx_out equals the host call's result,
 * order included; mask_bits equals bitmask_words(idx, n, False); the state block holds the state
 * np.random would be left in and is updated in place, so consecutive calls chain without the
 * host (openmsftl_amd/csrc/fc_perm.hip; pinned against NumPy in tests/test_perm_gpu.py).
 *   fc_mt_perm_plan: the segment jump polynomials for length n (host, cached; independent of n
 *     but for their count) into the DEVICE buffer `plan` (fc_mt_perm_plan_bytes(n));
 *     synchronises `stream`.
 *   fc_mt_perm_begin: (key: HOST uint32[624], pos in [0, 624]) into the DEVICE state block, its
 *     other words zeroed.
 *   fc_mt_permutation: one call of np.random.permutation(n)[:k] from the state block, on
 *     `stream`, no host synchronisation.  idx_out: DEVICE uint32[k] or NULL; mask_bits: DEVICE
 *     uint32[ceil(n/32)] (bits >= n zero) or NULL; not both NULL.  ws: DEVICE, 256-B aligned,
 *     fc_mt_perm_workspace_bytes(n).  max_words: the most outputs the call may consume (0, or
 *     anything above it: 2n + 4096; the expected need is ~1.4 n).  n <= 1 draws nothing.
 *     Fallback: if the draw needs more than max_words outputs (fallback = 1) or a trace runs
 *     into its loop bound (2), key and pos stay as they were, the outputs are unspecified and
 *     every later call on the block draws nothing: the caller makes the host call instead.
 *     k > n, n >= 2^31, a NULL plan / state / ws or two NULL outputs: FC_ERR_ARG; a short plan
 *     or workspace: FC_ERR_WORKSPACE (all checked before the GPU is touched).
 *   fc_mt_perm_timing (measurement, not thread-safe): on != 0 brackets the five stages of the
 *     following fc_mt_permutation calls (words, parse, link, trace, commit) with HIP events;
 *     stage_ms != NULL first waits for the last timed call and returns its five times. */
typedef struct {
  uint32_t key[624];              /* np.random.get_state()[1] after the calls so far */
  uint32_t pos;                   /* ... [2] */
  uint32_t fallback;              /* 0 ok, 1 word budget, 2 trace bound (sticky) */
  uint32_t rows_done;             /* calls that completed */
  uint32_t reserved;
  uint64_t consumed;              /* MT19937 outputs consumed, summed over those calls */
} fc_perm_state;
size_t fc_mt_perm_plan_bytes(uint64_t n);
int fc_mt_perm_plan(uint64_t n, void* plan, size_t plan_bytes, fc_stream_t stream);
size_t fc_mt_perm_workspace_bytes(uint64_t n);
int fc_mt_perm_begin(const uint32_t* key, uint32_t pos, void* state, fc_stream_t stream);
int fc_mt_permutation(const void* plan, size_t plan_bytes, uint64_t n, uint64_t k, uint64_t max_words,
                      void* state, uint32_t* idx_out, uint32_t* mask_bits, void* ws, size_t ws_bytes,
                      fc_stream_t stream);
int fc_mt_perm_timing(int on, double* stage_ms);

/* Ordering of in-kernel-waiting launches issued outside the library's own calls (a replayed
 * graph that contains fc_topk_encode / fc_topk_encode_dense / fc_topk_dense_f64_sampled):
 * fc_fused_order_begin(s) makes s wait for the device's last such launch; fc_fused_order_end(s)
 * marks s as holding the latest one. */
int fc_fused_order_begin(fc_stream_t stream);
int fc_fused_order_end(fc_stream_t stream);

/* ---- measurement: HIP events around selected kernels, on the stream they run on -------
 * mask: FC_TIME_* bits.  Between fc_timing_begin and fc_timing_end every launch of a
 * selected kernel class is bracketed by a hipEvent pair; fc_timing_end synchronises those
 * events and returns per-class total milliseconds and launch counts (arrays of 4). */
#define FC_TIME_COMPACT 1    /* k_compact: the single streaming pass over g (encode)   */
#define FC_TIME_DECODE 2     /* k_decode: dense decode / FedAVG decode-accumulate      */
#define FC_TIME_ENGINE 4     /* k_engine: exact threshold resolution                   */
#define FC_TIME_SAMPLE 8     /* k_sample: bracket estimation                           */
int fc_timing_begin(uint32_t mask);
int fc_timing_end(double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* FEDCODEC_H_ */
