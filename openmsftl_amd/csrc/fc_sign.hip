// fc_sign.hip — the scaled-sign codec with error feedback (EF-signSGD: Karimireddy, Rebjock,
// Stich, Jaggi, ICML 2019), its FedAVG fold and the majority vote over sign packets (signSGD with
// majority vote: Bernstein, Zhao, Azizzadenesheli, Anandkumar, ICLR 2019) for MI355X (gfx950).
// The packet layout and the host validator are in fc_sign_host.h.
//
//   a[t] = fl32(g[t] + e[t])  (g[t] without a residual)        one IEEE add
//   s    = fl32(sum_t (double)|a[t]| / (double)n)              fp64 sum in an order fixed by n
//   b[t] = the IEEE sign bit of a[t], bit t % 32 of word[t / 32]
//   q[t] = b[t] ? -s : +s;   e'[t] = fl32(a[t] - q[t])
//
// Encode, two launches, neither waits in-kernel for another workgroup:
//   k_sign_norm   grid from n alone (<= kSignNormGrid workgroups, grid-stride, two 16-B loads in
//                 flight per thread), per-workgroup fp64 partials, the last arriver (ticket) adds
//                 them in index order and writes the header.  4N (8N with a residual) read.
//   k_sign_pack   one wave per 256 consecutive elements: a 16-B load per lane (lane l: elements
//                 4l .. 4l + 3), the integer compare bits < 0 per component, one 64-lane ballot per
//                 component (four per 256 elements: one per 64 elements); lanes 0..7 each assemble
//                 one whole word from byte l of the four ballots (spread4) and store it; e' goes out
//                 as one 16-B store per lane.  4N (8N) read, N/8 (+ 4N) written.
// Batched encode (fc_sign_encode_batch), m clients per launch, client = blockIdx.y:
//   k_sign_encode1_batch  k_sign_norm's grid, loop and sum per client with k_sign_pack's ballots
//                 in the loop: header and words from ONE read, 4N (8N) + N/8 per client.
//   k_sign_resid_batch    only when e' is wanted: 4N (8N) read, 4N written per client.
// Decode: k_sign_decode, one 16-B store per lane.
// Fold and vote, three forms of bringing a client's words to the lanes (fc_sign_fold_form; the
//   results are the same bits, tools/sign_bench.py measures them side by side):
//   k_sign_reduce_lane (kSignFormLane, the default: fastest measured): lane =
//   one word = 32 consecutive coordinates, no bit crosses a lane.
//   k_sign_reduce: a wave owns 512 consecutive coordinates, lane l the eight coordinates
//   64 j + l: a client's 64-bit word j IS the lane mask of group j.  Per client the wave reads its
//   eight words wave-uniformly and per group does one v_cndmask (+c_i / -c_i by the mask) and one
//   add (fold), or one carry-in add (vote).  kSignFormScalar: scalar loads through the constant
//   address space; kSignFormVector: one vector load per four clients and v_readlane.
//   In all forms the clients' word pointers and c_i = fl32(w_i * s_i) are staged kSignBatch at a
//   time in LDS by the workgroup.  Bytes: m N/8 + 4N (+ 4N continuing).
#include "fc_state.h"
#include "fc_sign_host.h"

namespace fc {

constexpr int kSignNormGrid = 1024;            // fixed: the fp64 sum order depends on it
constexpr size_t kSignWsBytes = 64 + 8 * (size_t)kSignNormGrid;   // a ticket (own line) and the partials
constexpr int kSignNormUnroll = 2;             // 16-B loads in flight per thread (k_qsgd_norm's)
constexpr int kSignResidGrid = 8192;           // k_sign_resid_batch workgroups per client at most (k_sign_pack's)
constexpr int FC_SIGN_PACK_GRID = 8192;        // k_sign_pack / k_sign_decode workgroups at most
constexpr int kSignBatch = 256;                // clients staged in LDS per round of fold / vote
constexpr int kSignGroups = 8;                 // 64-coordinate groups per wave (512 coordinates)
constexpr int kSignTile = 64 * kSignGroups;
constexpr int kSignFormScalar = 0, kSignFormVector = 1, kSignFormLane = 2;
constexpr int kSignFormDefault = kSignFormLane;

__device__ __forceinline__ uint32_t sign_bit(float x) { return (int32_t)__float_as_uint(x) < 0; }

// ---- pass 1: s = fl32(sum |a| / n) (fp64, fixed order), header ------------------------------
template <bool RES>
__global__ __launch_bounds__(kBlock) void k_sign_norm(const float* __restrict__ g,
                                                      const float* __restrict__ e, uint64_t n,
                                                      double* partial, uint32_t* ticket,
                                                      fc_packet_hdr* hdr) {
  __shared__ double s_red[kBlock / 64];
  __shared__ uint32_t s_flag;
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  double acc = 0.0;
  const uint64_t n4 = n / 4, stride = (uint64_t)gridDim.x * kBlock;
  auto add4 = [&](float4 v, float4 r) {
    if (RES) v = make_float4(__fadd_rn(v.x, r.x), __fadd_rn(v.y, r.y), __fadd_rn(v.z, r.z), __fadd_rn(v.w, r.w));
    acc += (double)__builtin_fabsf(v.x); acc += (double)__builtin_fabsf(v.y);
    acc += (double)__builtin_fabsf(v.z); acc += (double)__builtin_fabsf(v.w);
  };
  uint64_t q = (uint64_t)blockIdx.x * kBlock + tid;
  for (; q + (kSignNormUnroll - 1) * stride < n4; q += kSignNormUnroll * stride) {
    float4 v[kSignNormUnroll], r[kSignNormUnroll];
#pragma unroll
    for (int u = 0; u < kSignNormUnroll; ++u) {
      v[u] = load4_full(g + 4 * (q + u * stride));
      r[u] = RES ? load4_full(e + 4 * (q + u * stride)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kSignNormUnroll; ++u) add4(v[u], r[u]);
  }
  for (; q < n4; q += stride)
    add4(load4_full(g + 4 * q), RES ? load4_full(e + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f));
  if (blockIdx.x == 0 && tid < (int)(n - 4 * n4)) {            // tail (< 4 elements)
    float t = g[4 * n4 + tid];
    if (RES) t = __fadd_rn(t, e[4 * n4 + tid]);
    acc += (double)__builtin_fabsf(t);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) s_red[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double b = 0.0;
    for (int i = 0; i < kBlock / 64; ++i) b += s_red[i];
    st_agent(reinterpret_cast<uint64_t*>(&partial[blockIdx.x]), (uint64_t)__double_as_longlong(b));
  }
  if (!last_block_arrive_sc1(ticket, gridDim.x, &s_flag)) return;
  // ---- last workgroup: fixed-order sum of the partials, header --------------------------
  double t = 0.0;
  for (uint32_t i = (uint32_t)tid; i < gridDim.x; i += kBlock)
    t += __longlong_as_double((long long)ld_agent(reinterpret_cast<const uint64_t*>(&partial[i])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __syncthreads();
  if (lane == 0) s_red[w] = t;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < kBlock / 64; ++i) sum += s_red[i];
    const float s = (float)(sum / (double)n);
    hdr->thresh = 0; hdr->lower = 0;
    hdr->n = (uint32_t)n; hdr->k = (uint32_t)n; hdr->n_entries = (uint32_t)n;
    hdr->index_bits = 0; hdr->codec = FC_CODEC_SIGN; hdr->status = FC_STATUS_OK;
    hdr->n_definite = 0; hdr->n_cand = 0;
    hdr->seed = 0; hdr->offset = 0; hdr->p = (double)s;
    hdr->chunk = 0; hdr->format = FC_FMT_SIGN; hdr->key_mode = 0;
    hdr->reserved[0] = hdr->reserved[1] = hdr->reserved[2] = 0;
    *ticket = 0;                                                  // for the next encode
  }
}

// ---- the batched encode (fc_sign_encode_batch): client = blockIdx.y --------------------------
// float4 load of [e0, e0 + 4) of a job's array with zero fill past n: load4 through the GLOBAL
// address space (the pointer comes out of the job table).
__device__ __forceinline__ float4 sign_load4(const FC_G float* p, uint64_t e0, uint64_t n) {
  if (e0 + 4 <= n) {
    const fc_f4v v = __builtin_nontemporal_load((fc_gf4v*)(p + e0));
    return make_float4(v.x, v.y, v.z, v.w);
  }
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e0 + 0 < n) r.x = p[e0 + 0];
  if (e0 + 1 < n) r.y = p[e0 + 1];
  if (e0 + 2 < n) r.z = p[e0 + 2];
  return r;
}
__device__ __forceinline__ float4 sign_add4(float4 a, float4 r) {
  return make_float4(__fadd_rn(a.x, r.x), __fadd_rn(a.y, r.y), __fadd_rn(a.z, r.z), __fadd_rn(a.w, r.w));
}

// The end of k_sign_norm for the batched kernel, statement for statement: every thread's fp64 sum
// acc to the wave, the workgroup, partial[blockIdx.x]; the last-arriving workgroup of the gridDim.x
// that count into *ticket adds the partials in index order, writes the header and clears the
// ticket.  (A copy: called from k_sign_norm too, hipcc allocated that kernel's registers
// differently, and fc_sign_encode's generated code stays as it was.)
__device__ __forceinline__ void sign_norm_finish(double acc, uint64_t n, double* partial,
                                                 uint32_t* ticket, fc_packet_hdr* hdr,
                                                 double* s_red, uint32_t* s_flag,
                                                 int tid, int lane, int w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) s_red[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double b = 0.0;
    for (int i = 0; i < kBlock / 64; ++i) b += s_red[i];
    st_agent(reinterpret_cast<uint64_t*>(&partial[blockIdx.x]), (uint64_t)__double_as_longlong(b));
  }
  if (!last_block_arrive_sc1(ticket, gridDim.x, s_flag)) return;
  // ---- last workgroup: fixed-order sum of the partials, header --------------------------
  double t = 0.0;
  for (uint32_t i = (uint32_t)tid; i < gridDim.x; i += kBlock)
    t += __longlong_as_double((long long)ld_agent(reinterpret_cast<const uint64_t*>(&partial[i])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __syncthreads();
  if (lane == 0) s_red[w] = t;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < kBlock / 64; ++i) sum += s_red[i];
    const float s = (float)(sum / (double)n);
    hdr->thresh = 0; hdr->lower = 0;
    hdr->n = (uint32_t)n; hdr->k = (uint32_t)n; hdr->n_entries = (uint32_t)n;
    hdr->index_bits = 0; hdr->codec = FC_CODEC_SIGN; hdr->status = FC_STATUS_OK;
    hdr->n_definite = 0; hdr->n_cand = 0;
    hdr->seed = 0; hdr->offset = 0; hdr->p = (double)s;
    hdr->chunk = 0; hdr->format = FC_FMT_SIGN; hdr->key_mode = 0;
    hdr->reserved[0] = hdr->reserved[1] = hdr->reserved[2] = 0;
    *ticket = 0;                                                  // for the next encode
  }
}

// One read for the header AND the words: k_sign_norm's grid and grid-stride loop with k_sign_pack's
// ballots inside it.  In k_sign_norm wave w of workgroup b loads at step j the 64 consecutive
// float4 from 256 b + 64 w + j * stride, stride = 256 * gridDim.x a multiple of 64: elements
// 256 t .. 256 t + 255 of tile t = 4 b + w + 4 gridDim.x j, lane l holding 4 l .. 4 l + 3, which is
// one k_sign_pack tile.  So the loop runs over the wave's tiles t < ceil(n / 256) (wave-uniform:
// every ballot sees 64 lanes), a lane adds its float4 exactly when k_sign_norm's thread would
// (q < n / 4, ascending j, .x .y .z .w; workgroup 0's tail scalars last), and the rest of the sum
// is sign_norm_finish: s has k_sign_norm's bits.  The lane that owns float4 index n / 4 loads the
// n % 4 tail elements for their bits alone.  Tiles below n / 256 are whole: two of them in flight
// per wave with no predicate, as k_sign_norm's unrolled loop.
template <bool RES>
__global__ __launch_bounds__(kBlock) void k_sign_encode1_batch(const fc_sign_job* __restrict__ jobs,
                                                               uint64_t n, uint64_t n_words, char* ws) {
  __shared__ double s_red[kBlock / 64];
  __shared__ uint32_t s_flag;
  const FC_G fc_sign_job* job = (const FC_G fc_sign_job*)jobs + blockIdx.y;
  const FC_G float* g = (const FC_G float*)job->g;
  const FC_G float* e = (const FC_G float*)job->res_in;
  FC_G uint32_t* words = (FC_G uint32_t*)job->words;
  char* wc = ws + (size_t)blockIdx.y * kSignWsBytes;
  const int tid = threadIdx.x;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t n4 = n / 4, whole = n / 256, tiles = (n + 255) / 256;
  const uint64_t tstep = (uint64_t)gridDim.x * kWaves;
  double acc = 0.0;
  auto sum4 = [&](float4 v) {
    acc += (double)__builtin_fabsf(v.x); acc += (double)__builtin_fabsf(v.y);
    acc += (double)__builtin_fabsf(v.z); acc += (double)__builtin_fabsf(v.w);
  };
  auto put = [&](uint64_t t, float4 a, bool all) {       // k_sign_pack's ballots and word stores
    const uint64_t m0 = __ballot(sign_bit(a.x)), m1 = __ballot(sign_bit(a.y));
    const uint64_t m2 = __ballot(sign_bit(a.z)), m3 = __ballot(sign_bit(a.w));
    if (lane < 8u && (all || t * 8 + lane < n_words)) {
      const uint32_t sh = 8u * lane;
      words[t * 8 + lane] = spread4((uint32_t)(m0 >> sh)) | (spread4((uint32_t)(m1 >> sh)) << 1) |
                            (spread4((uint32_t)(m2 >> sh)) << 2) | (spread4((uint32_t)(m3 >> sh)) << 3);
    }
  };
  uint64_t t = (uint64_t)blockIdx.x * kWaves + w;
  for (; t + tstep < whole; t += 2 * tstep) {
    const uint64_t e0 = t * 256 + 4 * lane, e1 = e0 + tstep * 256;
    float4 a0 = load4_full((const float*)(g + e0)), a1 = load4_full((const float*)(g + e1));
    if (RES) {
      const float4 r0 = load4_full((const float*)(e + e0)), r1 = load4_full((const float*)(e + e1));
      a0 = sign_add4(a0, r0); a1 = sign_add4(a1, r1);
    }
    sum4(a0); put(t, a0, true);
    sum4(a1); put(t + tstep, a1, true);
  }
  for (; t < tiles; t += tstep) {
    const uint64_t e0 = t * 256 + 4 * lane;
    float4 a = sign_load4(g, e0, n);
    if (RES) a = sign_add4(a, sign_load4(e, e0, n));
    if (t * 64 + lane < n4) sum4(a);
    put(t, a, false);
  }
  if (blockIdx.x == 0 && tid < (int)(n - 4 * n4)) {            // tail (< 4 elements), added last
    float x = g[4 * n4 + tid];
    if (RES) x = __fadd_rn(x, e[4 * n4 + tid]);
    acc += (double)__builtin_fabsf(x);
  }
  sign_norm_finish(acc, n, reinterpret_cast<double*>(wc + 64), reinterpret_cast<uint32_t*>(wc),
                   job->hdr, s_red, &s_flag, tid, (int)lane, tid >> 6);
}

// The second launch when e' is wanted: s from the client's own header, e' = fl32(a - (+-s)) as
// k_sign_pack<., true> computes it, one non-temporal 16-B store per float4, in k_sign_pack's
// geometry (a float4 per thread and step, at most 8192 workgroups per client).
template <bool RES>
__global__ __launch_bounds__(kBlock) void k_sign_resid_batch(const fc_sign_job* __restrict__ jobs,
                                                             uint64_t n) {
  const FC_G fc_sign_job* job = (const FC_G fc_sign_job*)jobs + blockIdx.y;
  const FC_G float* g = (const FC_G float*)job->g;
  const FC_G float* e = (const FC_G float*)job->res_in;
  FC_G float* eout = (FC_G float*)job->res_out;
  const float s = (float)((const FC_G fc_packet_hdr*)job->hdr)->p;
  const int tid = threadIdx.x;
  const uint64_t n4 = n / 4, stride = (uint64_t)gridDim.x * kBlock;
  auto resid = [&](float x) { return __fsub_rn(x, sign_bit(x) ? -s : s); };
  auto store = [&](uint64_t q, float4 a) {
    __builtin_nontemporal_store(fc_f4v{resid(a.x), resid(a.y), resid(a.z), resid(a.w)},
                                (FC_G fc_f4v*)(eout + 4 * q));
  };
  uint64_t q = (uint64_t)blockIdx.x * kBlock + tid;
  for (; q < n4; q += stride) {
    float4 a = load4_full((const float*)(g + 4 * q));
    if (RES) a = sign_add4(a, load4_full((const float*)(e + 4 * q)));
    store(q, a);
  }
  if (blockIdx.x == 0 && tid < (int)(n - 4 * n4)) {            // tail (< 4 elements)
    float x = g[4 * n4 + tid];
    if (RES) x = __fadd_rn(x, e[4 * n4 + tid]);
    eout[4 * n4 + tid] = resid(x);
  }
}

// ---- pass 2: the words (and e') ---------------------------------------------------------------
// wave = 256 consecutive elements; every element at or past n counts as +0.0 (bit 0), so tail
// bits and pad words come out zero.  n_words <= 8 * ceil(n / 256): every word has its tile.
template <bool RES, bool EOUT>
__global__ __launch_bounds__(kBlock) void k_sign_pack(const float* __restrict__ g,
                                                      const float* __restrict__ e,
                                                      float* __restrict__ eout, uint64_t n,
                                                      const fc_packet_hdr* __restrict__ hdr,
                                                      uint32_t* __restrict__ words, uint64_t n_words) {
  const float s = (float)hdr->p;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t tiles = (n + 255) / 256, wstride = (uint64_t)gridDim.x * kWaves;
  for (uint64_t t = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < tiles; t += wstride) {
    const uint64_t e0 = t * 256 + 4 * lane;
    float4 a = load4(g, e0, n);
    if (RES) {
      const float4 r = load4(e, e0, n);
      a = make_float4(__fadd_rn(a.x, r.x), __fadd_rn(a.y, r.y), __fadd_rn(a.z, r.z), __fadd_rn(a.w, r.w));
    }
    const uint32_t bx = sign_bit(a.x), by = sign_bit(a.y), bz = sign_bit(a.z), bw = sign_bit(a.w);
    const uint64_t m0 = __ballot(bx), m1 = __ballot(by), m2 = __ballot(bz), m3 = __ballot(bw);
    if (EOUT) {
      const float4 r = make_float4(__fsub_rn(a.x, bx ? -s : s), __fsub_rn(a.y, by ? -s : s),
                                   __fsub_rn(a.z, bz ? -s : s), __fsub_rn(a.w, bw ? -s : s));
      if (e0 + 4 <= n) {
        __builtin_nontemporal_store(fc_f4v{r.x, r.y, r.z, r.w}, reinterpret_cast<fc_f4v*>(eout + e0));
      } else {
        if (e0 + 0 < n) eout[e0 + 0] = r.x;
        if (e0 + 1 < n) eout[e0 + 1] = r.y;
        if (e0 + 2 < n) eout[e0 + 2] = r.z;
      }
    }
    if (lane < 8u && t * 8 + lane < n_words) {       // word l: elements 32 l .., lanes 8 l .. 8 l + 7
      const uint32_t sh = 8u * lane;
      words[t * 8 + lane] = spread4((uint32_t)(m0 >> sh)) | (spread4((uint32_t)(m1 >> sh)) << 1) |
                            (spread4((uint32_t)(m2 >> sh)) << 2) | (spread4((uint32_t)(m3 >> sh)) << 3);
    }
  }
}

// ---- decode: q[t] = b[t] ? -s : +s; thread = 4 elements, one 16-B store ----------------------
__global__ __launch_bounds__(kBlock) void k_sign_decode(const uint32_t* __restrict__ words,
                                                        const fc_packet_hdr* __restrict__ hdr,
                                                        uint64_t n, float* __restrict__ out) {
  const float s = (float)hdr->p;
  const uint64_t quads = (n + 3) / 4, stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < quads; q += stride) {
    const uint32_t nib = words[q >> 3] >> (4u * (uint32_t)(q & 7));
    const float4 v = make_float4(nib & 1u ? -s : s, nib & 2u ? -s : s, nib & 4u ? -s : s, nib & 8u ? -s : s);
    const uint64_t e = q * 4;
    if (e + 4 <= n) {
      __builtin_nontemporal_store(fc_f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<fc_f4v*>(out + e));
    } else {
      if (e + 0 < n) out[e + 0] = v.x;
      if (e + 1 < n) out[e + 1] = v.y;
      if (e + 2 < n) out[e + 2] = v.z;
    }
  }
}

// ---- fold and vote -------------------------------------------------------------------------
struct SignArgs {
  const fc_packet_view* views;
  int m, acc_in;
  uint64_t n, n_words;
  float eta;                       // vote
  float* out;
};
struct SignClient {                // 16 bytes in LDS: one ds_read_b128
  uint64_t words;                  // the client's word pointer
  float c;                         // fl32(w_i * s_i) (fold)
  uint32_t pad;
};

typedef __attribute__((address_space(4))) const uint64_t fc_cu64;

// The eight 64-bit words of tile t of one client, wave-uniform.  full: all sixteen uint32 words
// exist (t * 16 + 16 <= n_words); else word pairs past n_words (a multiple of 4) read as zero.
__device__ __forceinline__ void sign_words_scalar(uint64_t ptr, uint64_t t, uint64_t n_words,
                                                  bool full, uint64_t (&mk)[kSignGroups]) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)ptr);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(ptr >> 32));
  fc_cu64* wp = (fc_cu64*)(((uint64_t)hi << 32) | lo) + t * kSignGroups;
  if (full) {
#pragma unroll
    for (int j = 0; j < kSignGroups; ++j) mk[j] = wp[j];
  } else {
#pragma unroll
    for (int j = 0; j < kSignGroups; ++j)
      mk[j] = (t * kSignGroups + j) * 2 + 2 <= n_words ? wp[j] : 0ull;
  }
}

// VOTE: out = -eta / +eta / +0 by the count of set bits; else the FedAVG fold.  FORM: how the
// words reach the wave.  One wave per tile of 512 coordinates, four tiles per workgroup.
template <bool VOTE, int FORM>
__global__ __launch_bounds__(kBlock) void k_sign_reduce(SignArgs a) {
  __shared__ SignClient s_cl[kSignBatch];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n = a.n, tiles = (n + kSignTile - 1) / kSignTile;
  // (readfirstlane: the compiler must know the tile is wave-uniform, or the word loads below
  // sit in divergent control flow and become vector loads)
  const uint64_t t = (uint64_t)blockIdx.x * kWaves +
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool live = t < tiles;                                      // wave-uniform
  const bool full = live && (t + 1) * (2 * kSignGroups) <= a.n_words;
  const uint64_t c0 = t * kSignTile + lane;                         // coordinate of group 0
  float acc[kSignGroups];
  uint32_t cnt[kSignGroups];
#pragma unroll
  for (int j = 0; j < kSignGroups; ++j) {
    acc[j] = 0.f;                                                   // from +0 (np.sum, k_wsum)
    cnt[j] = 0u;
    if (!VOTE && a.acc_in && live && c0 + 64 * j < n) acc[j] = a.out[c0 + 64 * j];
  }
  for (int i0 = 0; i0 < a.m; i0 += kSignBatch) {
    const int nb = a.m - i0 < kSignBatch ? a.m - i0 : kSignBatch;
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += kBlock) {
      const FC_G fc_packet_view* v = (const FC_G fc_packet_view*)a.views + (i0 + i);
      SignClient c;
      c.words = (uint64_t)v->bitmap;
      c.c = VOTE ? 0.f : __fmul_rn(v->weight, (float)((const FC_G fc_packet_hdr*)v->hdr)->p);
      c.pad = 0u;
      s_cl[i] = c;
    }
    __syncthreads();
    if (!live) continue;
    if (FORM == kSignFormScalar) {
      // client i + 1's words are requested before client i's are used: a scalar load's latency
      // hides under the sixteen vector instructions of the client before
      SignClient c = s_cl[0];
      uint64_t mk[kSignGroups];
      sign_words_scalar(c.words, t, a.n_words, full, mk);
      for (int i = 0; i < nb; ++i) {
        SignClient cn = c;
        uint64_t nx[kSignGroups];
#pragma unroll
        for (int j = 0; j < kSignGroups; ++j) nx[j] = 0ull;
        if (i + 1 < nb) {
          cn = s_cl[i + 1];
          sign_words_scalar(cn.words, t, a.n_words, full, nx);
        }
#pragma unroll
        for (int j = 0; j < kSignGroups; ++j) {
          const bool neg = __builtin_amdgcn_inverse_ballot_w64(mk[j]);
          if (VOTE) cnt[j] += neg ? 1u : 0u;
          else acc[j] = __fadd_rn(acc[j], neg ? -c.c : c.c);
          mk[j] = nx[j];
        }
        c = cn;
      }
    } else {
      // lane l: uint32 word l % 16 of the tile of client i + l / 16: four clients per load
      const uint64_t wi = t * (2 * kSignGroups) + (lane & 15u);
      for (int i = 0; i < nb; i += 4) {
        const int mine = i + (int)(lane >> 4);
        uint32_t v = 0u;
        if (mine < nb && wi < a.n_words) v = ((const FC_G uint32_t*)s_cl[mine].words)[wi];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          if (i + d >= nb) break;
          const float cc = s_cl[i + d].c;
#pragma unroll
          for (int j = 0; j < kSignGroups; ++j) {
            const uint64_t mk = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)v, 16 * d + 2 * j) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)v, 16 * d + 2 * j + 1) << 32);
            const bool neg = __builtin_amdgcn_inverse_ballot_w64(mk);
            if (VOTE) cnt[j] += neg ? 1u : 0u;
            else acc[j] = __fadd_rn(acc[j], neg ? -cc : cc);
          }
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < kSignGroups; ++j) {
    if (c0 + 64 * j >= n) continue;
    if (VOTE) {
      const uint32_t twice = 2u * cnt[j], m = (uint32_t)a.m;
      a.out[c0 + 64 * j] = twice > m ? -a.eta : twice < m ? a.eta : 0.f;
    } else {
      a.out[c0 + 64 * j] = acc[j];
    }
  }
}

// The per-lane form (kSignFormLane): lane = one uint32 word = 32 consecutive coordinates, so a
// client's words reach the wave as one coalesced 256-B load and no bit ever crosses a lane.  Per
// coordinate and client: the bit spread to a full mask (v_bfe_i32), the select between -c_i and
// +c_i by that mask (v_bfi_b32) and the add; the vote extracts the bit (v_bfe_u32) and adds it.
// Four clients' words are requested before the first is used.  The 32 sums of a lane go out as
// eight 16-B stores.
template <bool VOTE>
__global__ __launch_bounds__(kBlock) void k_sign_reduce_lane(SignArgs a) {
  __shared__ SignClient s_cl[kSignBatch];
  constexpr int D = 4;
  const uint64_t n = a.n;
  const uint64_t wi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;   // this lane's word
  const uint64_t c0 = 32 * wi;                                       // its first coordinate
  const bool live = wi < a.n_words && c0 < n;
  const bool whole = live && c0 + 32 <= n;
  float acc[32];
  uint32_t cnt[32];
#pragma unroll
  for (int b = 0; b < 32; ++b) { acc[b] = 0.f; cnt[b] = 0u; }       // from +0 (np.sum, k_wsum)
  if (!VOTE && a.acc_in && live) {
    if (whole) {
#pragma unroll
      for (int b = 0; b < 32; b += 4) {
        const fc_f4v v = *(const FC_G fc_f4v*)(a.out + c0 + b);
        acc[b] = v.x; acc[b + 1] = v.y; acc[b + 2] = v.z; acc[b + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int b = 0; b < 32; ++b) if (c0 + b < n) acc[b] = a.out[c0 + b];
    }
  }
  for (int i0 = 0; i0 < a.m; i0 += kSignBatch) {
    const int nb = a.m - i0 < kSignBatch ? a.m - i0 : kSignBatch;
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += kBlock) {
      const FC_G fc_packet_view* v = (const FC_G fc_packet_view*)a.views + (i0 + i);
      SignClient c;
      c.words = (uint64_t)v->bitmap;
      c.c = VOTE ? 0.f : __fmul_rn(v->weight, (float)((const FC_G fc_packet_hdr*)v->hdr)->p);
      c.pad = 0u;
      s_cl[i] = c;
    }
    __syncthreads();
    if (!live) continue;
    for (int i = 0; i < nb; i += D) {
      uint32_t w[D];
      float c[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        w[d] = 0u; c[d] = 0.f;
        if (i + d < nb) {
          w[d] = ((const FC_G uint32_t*)s_cl[i + d].words)[wi];
          c[d] = s_cl[i + d].c;
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if (i + d >= nb) break;
        const uint32_t pos = __float_as_uint(c[d]), neg = pos ^ 0x80000000u;
#pragma unroll
        for (int b = 0; b < 32; ++b) {
          if (VOTE) {
            cnt[b] += (w[d] >> b) & 1u;
          } else {
            const uint32_t mk = (uint32_t)((int32_t)(w[d] << (31 - b)) >> 31);    // bit b everywhere
            acc[b] = __fadd_rn(acc[b], __uint_as_float((mk & neg) | (~mk & pos)));
          }
        }
      }
    }
  }
  if (!live) return;
  if (VOTE) {
    const uint32_t m = (uint32_t)a.m;
#pragma unroll
    for (int b = 0; b < 32; ++b) acc[b] = 2u * cnt[b] > m ? -a.eta : 2u * cnt[b] < m ? a.eta : 0.f;
  }
  if (whole) {
#pragma unroll
    for (int b = 0; b < 32; b += 4)
      *(FC_G fc_f4v*)(a.out + c0 + b) = fc_f4v{acc[b], acc[b + 1], acc[b + 2], acc[b + 3]};
  } else {
#pragma unroll
    for (int b = 0; b < 32; ++b) if (c0 + b < n) a.out[c0 + b] = acc[b];
  }
}

}  // namespace fc

using namespace fc;

namespace { int g_sign_form = kSignFormDefault; }

extern "C" {

uint64_t fc_sign_words(uint64_t n) { return sign_words(n); }

size_t fc_sign_workspace_bytes(uint64_t n) {
  (void)n;
  return kSignWsBytes;
}

size_t fc_sign_batch_workspace_bytes(uint64_t n, int m) {
  return (size_t)(m < 1 ? 1 : m) * fc_sign_workspace_bytes(n);
}

int fc_sign_wire_validate(const void* host_bytes, size_t len, uint64_t n_expected) {
  return fc::sign_wire_validate(host_bytes, len, n_expected, g_err, sizeof g_err);
}

static bool sign_overlap(const float* a, const float* b, uint64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)(4 * n);
  return x < y + len && y < x + len;
}

int fc_sign_encode(const float* g, const float* res_in, float* res_out, uint64_t n, uint32_t* words,
                   uint64_t n_words, fc_packet_hdr* hdr, void* ws, size_t ws_bytes,
                   fc_stream_t stream) {
  FC_CHECK(g && words && hdr && ws, "NULL argument");
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)g & 15) == 0 && ((uintptr_t)res_in & 15) == 0 && ((uintptr_t)res_out & 15) == 0 &&
               ((uintptr_t)words & 15) == 0,
           "g, res_in, res_out and words must be 16-byte aligned");
  FC_CHECK(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
  FC_CHECK(n_words >= fc_sign_words(n), "n_words %llu < %llu needed", (unsigned long long)n_words,
           (unsigned long long)fc_sign_words(n));
  FC_CHECK(!res_out || (!sign_overlap(res_out, g, n) && (!res_in || !sign_overlap(res_out, res_in, n))),
           "res_out must not overlap g or res_in");
  if (ws_bytes < fc_sign_workspace_bytes(n))
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes, fc_sign_workspace_bytes(n));
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(ws);
  uint64_t ng = (n / 4 + kBlock - 1) / kBlock;                 // fixed for a given n
  if (ng < 1) ng = 1;
  if (ng > (uint64_t)kSignNormGrid) ng = kSignNormGrid;
  double* partial = reinterpret_cast<double*>(w + 64);
  uint32_t* ticket = reinterpret_cast<uint32_t*>(w);
  {
    TimedLaunch t(FC_TIME_SAMPLE, s);
    if (res_in) hipLaunchKernelGGL(k_sign_norm<true>, dim3((uint32_t)ng), dim3(kBlock), 0, s, g, res_in, n, partial, ticket, hdr);
    else hipLaunchKernelGGL(k_sign_norm<false>, dim3((uint32_t)ng), dim3(kBlock), 0, s, g, res_in, n, partial, ticket, hdr);
    FC_LAUNCHED("k_sign_norm");
  }
  const uint64_t nw = fc_sign_words(n);                        // the packet's words, no more
  const dim3 grid(stream_grid((n + 255) / 256 * 64, FC_SIGN_PACK_GRID)), blk(kBlock);
  TimedLaunch t(FC_TIME_COMPACT, s);
  if (res_in && res_out) hipLaunchKernelGGL((k_sign_pack<true, true>), grid, blk, 0, s, g, res_in, res_out, n, hdr, words, nw);
  else if (res_in) hipLaunchKernelGGL((k_sign_pack<true, false>), grid, blk, 0, s, g, res_in, res_out, n, hdr, words, nw);
  else if (res_out) hipLaunchKernelGGL((k_sign_pack<false, true>), grid, blk, 0, s, g, res_in, res_out, n, hdr, words, nw);
  else hipLaunchKernelGGL((k_sign_pack<false, false>), grid, blk, 0, s, g, res_in, res_out, n, hdr, words, nw);
  FC_LAUNCHED("k_sign_pack");
  return FC_OK;
}

int fc_sign_encode_batch(const fc_sign_job* jobs_dev, int m, uint64_t n, int has_res_in,
                         int has_res_out, void* ws, size_t ws_bytes, fc_stream_t stream) {
  FC_CHECK(jobs_dev && ws, "NULL argument");
  FC_CHECK(m >= 1 && m <= 65535, "m=%d outside [1, 65535]", m);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)ws & 7) == 0,
           "the job table and the workspace must be 8-byte aligned");
  if (ws_bytes < fc_sign_batch_workspace_bytes(n, m))
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes,
                fc_sign_batch_workspace_bytes(n, m));
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(ws);
  uint64_t ng = (n / 4 + kBlock - 1) / kBlock;                 // fc_sign_encode's: fixed for a given n
  if (ng < 1) ng = 1;
  if (ng > (uint64_t)kSignNormGrid) ng = kSignNormGrid;
  const uint64_t nw = fc_sign_words(n);
  const dim3 blk(kBlock);
  {
    TimedLaunch t(FC_TIME_SAMPLE, s);
    const dim3 grid((uint32_t)ng, (uint32_t)m);
    if (has_res_in) hipLaunchKernelGGL(k_sign_encode1_batch<true>, grid, blk, 0, s, jobs_dev, n, nw, w);
    else hipLaunchKernelGGL(k_sign_encode1_batch<false>, grid, blk, 0, s, jobs_dev, n, nw, w);
    FC_LAUNCHED("k_sign_encode1_batch");
  }
  if (!has_res_out) return FC_OK;
  uint64_t nr = (n / 4 + kBlock - 1) / kBlock;
  if (nr < 1) nr = 1;
  if (nr > (uint64_t)kSignResidGrid) nr = kSignResidGrid;
  TimedLaunch t(FC_TIME_COMPACT, s);
  const dim3 grid((uint32_t)nr, (uint32_t)m);
  if (has_res_in) hipLaunchKernelGGL(k_sign_resid_batch<true>, grid, blk, 0, s, jobs_dev, n);
  else hipLaunchKernelGGL(k_sign_resid_batch<false>, grid, blk, 0, s, jobs_dev, n);
  FC_LAUNCHED("k_sign_resid_batch");
  return FC_OK;
}

int fc_sign_decode(const fc_packet_view* pkt, uint64_t n, float* out, fc_stream_t stream) {
  FC_CHECK(pkt && out && pkt->bitmap && pkt->hdr, "NULL argument");
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)out & 15) == 0 && ((uintptr_t)pkt->bitmap & 15) == 0,
           "out and the words must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch t(FC_TIME_DECODE, s);
  hipLaunchKernelGGL(k_sign_decode, dim3(stream_grid((n + 3) / 4, FC_SIGN_PACK_GRID)), dim3(kBlock), 0, s,
                     pkt->bitmap, pkt->hdr, n, out);
  FC_LAUNCHED("k_sign_decode");
  return FC_OK;
}

static int sign_reduce(const fc_packet_view* views_dev, int m, uint64_t n, float eta, float* out,
                       int continue_sum, bool vote, fc_stream_t stream) {
  FC_CHECK(views_dev && out, "NULL argument");
  FC_CHECK(m >= 1 && m <= 65535, "m=%d outside [1, 65535]", m);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
  SignArgs a;
  memset(&a, 0, sizeof a);
  a.views = views_dev; a.m = m; a.acc_in = continue_sum != 0; a.n = n; a.n_words = fc_sign_words(n);
  a.eta = eta; a.out = out;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t tiles = (n + kSignTile - 1) / kSignTile;
  const dim3 grid((uint32_t)((tiles + kWaves - 1) / kWaves)), blk(kBlock);
  TimedLaunch t(FC_TIME_DECODE, s);
  if (g_sign_form == kSignFormLane) {
    const dim3 lgrid((uint32_t)((a.n_words + kBlock - 1) / kBlock));
    if (vote) hipLaunchKernelGGL(k_sign_reduce_lane<true>, lgrid, blk, 0, s, a);
    else hipLaunchKernelGGL(k_sign_reduce_lane<false>, lgrid, blk, 0, s, a);
    FC_LAUNCHED("k_sign_reduce_lane");
    return FC_OK;
  }
  const bool vec = g_sign_form == kSignFormVector;
  if (vote) {
    if (vec) hipLaunchKernelGGL((k_sign_reduce<true, kSignFormVector>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((k_sign_reduce<true, kSignFormScalar>), grid, blk, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_sign_reduce<false, kSignFormVector>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((k_sign_reduce<false, kSignFormScalar>), grid, blk, 0, s, a);
  }
  FC_LAUNCHED("k_sign_reduce");
  return FC_OK;
}

int fc_sign_fold(const fc_packet_view* views_dev, int m, uint64_t n, float* out, int continue_sum,
                 fc_stream_t stream) {
  return sign_reduce(views_dev, m, n, 0.f, out, continue_sum, false, stream);
}

int fc_sign_vote(const fc_packet_view* views_dev, int m, uint64_t n, float eta, float* out,
                 fc_stream_t stream) {
  return sign_reduce(views_dev, m, n, eta, out, 0, true, stream);
}

int fc_sign_fold_form(int form) {
  FC_CHECK(form >= -1 && form <= kSignFormLane, "bad form %d", form);
  g_sign_form = form == -1 ? kSignFormDefault : form;
  return FC_OK;
}

}  // extern "C"
