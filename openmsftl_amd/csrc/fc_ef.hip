// fc_ef.hip — error feedback (residual accumulation) for top-k: the fused accumulate + encode.
//
// A client that sparsifies with 'top' keeps what it dropped: a = fl32(g + e) is encoded instead
// of g, and the new residual is e' = selected ? +0 : a (compression.py:31-37 has no such state;
// one Compression object per client, client.py:23, is where it lives).  Composed from the other
// entry points that is a = g + e (12N bytes), encode (4N), decode (4N + packet), e' = a - q
// (12N); here it is ONE pass over g and e that writes e' and the packet:
//
//   k_sample1_ef        k_sample1's bracket, its sample keyed on g + e (sample_body over EfSrc)
//   k_compact_mag1_ef   k_compact_mag1's chunk pass on a = g + e (16 elements per lane, summed in
//                       registers), the packet side unchanged (compact_mag_body), plus e' with the
//                       layout of the loads: +0 above the bracket, a everywhere else — whether a
//                       bracket candidate is selected is only known at T64
//   k_resolve<.., EF>   fc_topk.hip: exact T64, and +0 into e' at the candidates at or above it
//
// Nothing here waits in-kernel for another workgroup (last-arriver tickets only), so the call
// runs beside any other kernel.  The exact fallback (header status RETRY_EXACT, whose e' is not
// valid) is fc_ef_sum -> fc_topk_encode_exact on the sum -> fc_ef_clear.
//
// The batched form (fc_topk_encode_ef_batch) is fc_topk_encode_batch's chain on a_c = g_c + e_c
// for m clients, the pairs (e_c, e'_c) in a second device table (fc_ef_job) beside the jobs:
//
//   k_pilot_ef            k_pilot over EfSrc: one workgroup per client, the window in win_flag
//   k_sample1_ef_batch    k_sample1<kKeyMag, true>'s body over EfSrc, grid.y = client
//   k_compact_mag1_ef_batch   the pass above in k_compact_mag1's batched geometry (mag_item_of)
//   k_resolve<true>, k_resolve<false, EF>   grid.y = client, e' from ef[client].res_out
#include "fc_state.h"

namespace fc {

// The sample of a = g + e: sample_body / pilot_window only hand their source to load4_sample,
// so the pair travels as a pointer to this record (a kernel-local object: its two fields stay
// in registers once the calls are inlined).
struct EfSrc {
  const float* g;
  const float* e;
};
__device__ __forceinline__ float4 load4_sample(const EfSrc* __restrict__ s, uint64_t e, uint64_t n) {
  const float4 a = load4_sample(s->g, e, n), b = load4_sample(s->e, e, n);
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__global__ __launch_bounds__(kBlock, 8) void k_sample1_ef(const float* __restrict__ g,
                                                       const float* __restrict__ e, SamplePlan P,
                                                       WsPtrs W, uint32_t ib, fc_packet_hdr* hdr,
                                                       HdrInit HI) {
  __shared__ SampleShared sm;
  const EfSrc src{g, e};
  sample_body<kKeyMag, false, EfSrc, false>(&src, P, 0ull, 0ull, W, ib, hdr, HI, blockIdx.x, gridDim.x,
                                            false, sm, 0u);
}

// The batched pilot and sample: k_pilot / k_sample1<kKeyMag, true> with the source of client
// blockIdx.x / blockIdx.y taken from the two job tables.  Magnitude keys: no seed, no offset.
__global__ __launch_bounds__(kBlock) void k_pilot_ef(SamplePlan P, WsPtrs W, const fc_encode_job* jobs,
                                                     const fc_ef_job* ef, uint64_t ws_stride) {
  __shared__ uint32_t h[kHistBins];
  __shared__ uint32_t s_tmp[8], s_out[4];
  const EfSrc src{jobs[blockIdx.x].g, ef[blockIdx.x].res_in};
  W = ws_shift(W, (uint64_t)blockIdx.x * ws_stride);
  for (int b = threadIdx.x; b < kHistBins; b += kBlock) h[b] = 0;
  float4 xs[kSampleSegs];
  uint32_t es[kSampleSegs], ls[kSampleSegs];
#pragma unroll
  for (int q = 0; q < kSampleSegs; ++q) { xs[q] = make_float4(0.f, 0.f, 0.f, 0.f); es[q] = ls[q] = 0; }
  const FineWin F = pilot_window<kKeyMag, false, EfSrc>(&src, P, 0ull, 0ull, h, s_tmp, s_out, false, xs, es, ls);
  if (threadIdx.x == 0) W.st->win_flag = 0x80000000u | ((F.khi >> 19) << 12) | (F.klo >> 19);
}

__global__ __launch_bounds__(kBlock, 8) void k_sample1_ef_batch(SamplePlan P, WsPtrs W, uint32_t ib,
                                                             HdrInit HI, const fc_encode_job* jobs,
                                                             const fc_ef_job* ef, uint64_t ws_stride) {
  __shared__ SampleShared sm;
  const fc_encode_job& J = jobs[blockIdx.y];
  const EfSrc src{J.g, ef[blockIdx.y].res_in};
  W = ws_shift(W, (uint64_t)blockIdx.y * ws_stride);
  sample_body<kKeyMag, false, EfSrc, true>(&src, P, 0ull, 0ull, W, ib, J.hdr, HI, blockIdx.x, gridDim.x,
                                           false, sm, 0u);
}

// The two residual pointers travel beside CompactArgs (which the other compactions share).
struct EfArgs {
  const float* res_in;
  float* res_out;
};

// x[] += the same elements of e (mag_load's layout and clamping), half of them in flight at a
// time: with all 16 beside the 16 of g the kernel spilled VGPRs at its 64-register budget
template <int NW>
__device__ __forceinline__ void ef_add(const float* e, uint32_t chunk, uint64_t n,
                                       float (&x)[MagGeo<NW>::kQ]) {
  constexpr int NQ = MagGeo<NW>::kQ, IS = MagGeo<NW>::kIStride, H = NQ / 2;
  const uint32_t base = chunk * (uint32_t)kChunk;
  typedef __attribute__((address_space(1))) const float gf;
  const uint32_t l0 = (uint32_t)((threadIdx.x >> 6) * 256 + lane_id());
  const bool part = (uint64_t)base + kChunk > n;
  const uint32_t last = part ? (uint32_t)(n - 1) - base : (uint32_t)kChunk - 1u;
  gf* ep = (gf*)e + base;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float r[H];
#pragma unroll
    for (int q = 0; q < H; ++q) {
      const uint32_t o = l0 + ((h * H + q) >> 2) * IS + ((h * H + q) & 3) * 64;
      r[q] = part ? ep[min(o, last)] : __builtin_nontemporal_load(ep + o);
    }
#pragma unroll
    for (int q = 0; q < H; ++q) x[h * H + q] = x[h * H + q] + r[q];
  }
}

// One 512-thread workgroup per chunk (grid = nchunks), k_compact_mag1's geometry.
//   fast chunk   e' leaves first (non-temporal, the loads' layout), then the packet side runs on
//                x[] = a exactly as for a gradient;
//   exact chunk  (partial last chunk, the chunk holding L64's index tie-break, thresholds at +inf
//                bits) compact_mag_body<false> re-reads values through MagOut::g: a is stored to
//                e' first and MagOut::g points there (each lane re-reads only what it stored
//                itself), then the elements above the bracket are overwritten with +0.
// (client: the batched launch's; a lone call's is 0 with a0.jobs == nullptr)
__device__ __forceinline__ void compact_mag_ef_wg(const CompactArgs& a0, const float* g,
                                                  const EfArgs& ef, uint32_t client, uint32_t chunk) {
  constexpr int NW = 8, NQ = MagGeo<NW>::kQ, IS = MagGeo<NW>::kIStride;
  __shared__ __attribute__((aligned(16))) MagShared sh;
  const int tid = threadIdx.x;
  float x[NQ];
  mag_load<NW>(g, chunk, a0.n, x);
  ef_add<NW>(ef.res_in, chunk, a0.n, x);                    // a = fl32(g + e)
  const MagState st = mag_state(mag_S(a0, client));
  MagOut o = mag_out(a0, client);
  FC_G float* ro = (FC_G float*)ef.res_out;
  const uint32_t base = chunk * (uint32_t)kChunk;
  const uint32_t l0 = (uint32_t)((tid >> 6) * 256 + lane_id());
  // the chunk's predicate parameters: compact_mag_item's
  const bool full = (uint64_t)base + kChunk <= a0.n;
  const bool none = st.L64 == kSelectNothing;
  MagPred P;
  P.t_lo = st.t_lo; P.t_hi = st.t_hi; P.cand_on = st.cand_on; P.n32 = (uint32_t)a0.n;
  P.Lk = none ? 0xffffffffu : (uint32_t)(st.L64 >> a0.ib);
  P.Li = none ? 0xffffffffu : (uint32_t)(st.L64 & ((1ull << a0.ib) - 1));
  const uint32_t Lk_eff = base >= P.Li ? P.Lk : P.Lk + 1u;
  const bool tie_inside = !none && base < P.Li && (uint64_t)base + kChunk > P.Li;
  const bool fast = full && !none && !tie_inside && Lk_eff <= 0x7f800000u;
  P.T_list = __uint_as_float(fast ? Lk_eff : 0u);
  P.cand_all = P.t_hi >= 0x7f800001u;
  P.T_hi = __uint_as_float(P.cand_all ? 0x7f800000u : P.t_hi);
  if (fast) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      // above the bracket (listed, not a candidate): selected whatever T64 turns out to be
      const bool sel = mag_listed<true>(P, x[q]) && !(P.cand_on != 0 && mag_cand<true>(P, x[q]));
      __builtin_nontemporal_store(sel ? 0.0f : x[q], ro + base + l0 + (q >> 2) * IS + (q & 3) * 64);
    }
    compact_mag_body<true, MagShared, NW, false, false, true, false>(o, P, x, sh, chunk, st.sbin);
  } else if (none) {                                       // k = 0: nothing listed, e' = a
    MagShared::barrier();
    if (tid == 0) {
      o.cnt[chunk] = 0;
      if (o.qoff) o.qoff[chunk] = 0;
      o.ccnt[chunk] = 0;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const uint32_t e = base + l0 + (q >> 2) * IS + (q & 3) * 64;
      if (e < P.n32) ro[e] = x[q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const uint32_t e = base + l0 + (q >> 2) * IS + (q & 3) * 64;
      if (e < P.n32) ro[e] = x[q];
    }
    o.g = (const FC_G float*)ef.res_out;
    mag_exact_bits<NW>(P, x, base + l0);
    compact_mag_body<false, MagShared, NW, false, false, true, false>(o, P, x, sh, chunk, st.sbin);
#pragma unroll
    for (int q = 0; q < NQ; ++q)                          // bit 1 listed, bit 0 candidate
      if (__float_as_uint(x[q]) == 2u) ro[base + l0 + (q >> 2) * IS + (q & 3) * 64] = 0.0f;
  }
}
__global__ __launch_bounds__(kCBlock, FC_MAG1_WAVES_PER_EU) void k_compact_mag1_ef(CompactArgs a0,
                                                                                  EfArgs ef) {
  compact_mag_ef_wg(a0, a0.g, ef, 0u, blockIdx.x);
}

// The batched launch: k_compact_mag1's geometry (mag_item_of: 64 clients' chunks interleaved in a
// 3-D grid, the linear grid above 65,535 chunks), the client's gradient and residual pair read
// from the two tables in one scalar round trip ahead of the loads (through the scalar cache, as
// mag_out reads the job: no kernel of the chain writes either table).
__device__ __forceinline__ void ef_item_ptrs(const CompactArgs& a0, const fc_ef_job* ef, uint32_t client,
                                             const float*& g, EfArgs& r) {
  fc_u32x2 gv;
  fc_u32x4 ev;
  asm volatile("s_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx4 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(gv), "=&s"(ev) : "s"(&a0.jobs[client].g), "s"(&ef[client]) : "memory");
  g = as_ptr<const float>(gv.x, gv.y);
  r.res_in = as_ptr<const float>(ev.x, ev.y);
  r.res_out = as_ptr<float>(ev.z, ev.w);
}
__global__ __launch_bounds__(kCBlock, FC_MAG1_WAVES_PER_EU) void k_compact_mag1_ef_batch(
    CompactArgs a0, const fc_ef_job* ef) {
  uint32_t client, chunk;
  mag_item_of(a0, client, chunk);
  if (client >= a0.m) return;                            // a partial last group
  const float* g;
  EfArgs r;
  ef_item_ptrs(a0, ef, client, g, r);
  compact_mag_ef_wg(a0, g, r, client, chunk);
}

// ---- the exact fallback's two streaming passes -------------------------------------------
// out = fl32(g + e): one float4 per thread and step, the tail element by element
__global__ __launch_bounds__(kBlock) void k_ef_sum(const float* __restrict__ g,
                                                   const float* __restrict__ e,
                                                   float* __restrict__ out, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock * 4;
  for (uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      const float4 a = load4_full(g + i), b = load4_full(e + i);
      fc_f4v v;
      v.x = a.x + b.x; v.y = a.y + b.y; v.z = a.z + b.z; v.w = a.w + b.w;
      __builtin_nontemporal_store(v, (FC_G fc_f4v*)(out + i));
    } else {
      for (uint64_t j = i; j < n; ++j) out[j] = g[j] + e[j];
    }
  }
}

// +0 into out at every packet entry the decoders keep (comp >= T64): chunk c's entries are
// [c * kChunk, c * kChunk + cnt[c]) of idx / val, as every decoder walks them
struct EfClearArgs {
  const uint16_t* idx;
  const float* val;
  const uint32_t* cnt;
  const fc_packet_hdr* hdr;
  float* out;
  uint64_t n;
  uint32_t ib, nchunks;
};
__global__ __launch_bounds__(kBlock) void k_ef_clear(EfClearArgs a) {
  const uint64_t T = a.hdr->thresh;
  for (uint32_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const uint32_t m = min(a.cnt[c], (uint32_t)kChunk);
    const uint64_t slot = (uint64_t)c * kChunk;
    for (uint32_t t = threadIdx.x; t < m; t += kBlock) {
      const uint64_t e = slot + a.idx[slot + t];
      if (e < a.n && comp_of(mag_key(a.val[slot + t]), (uint32_t)e, a.ib) >= T) a.out[e] = 0.0f;
    }
  }
}

}  // namespace fc

// ---- entry points (include/fedcodec.h) -------------------------------------------------
static bool ef_overlap(const void* a, const void* b, uint64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * 4;
  return x < y + len && y < x + len;
}

extern "C" {

int fc_ef_sum(const float* g, const float* res_in, float* res_out, uint64_t n, fc_stream_t stream) {
  FC_CHECK(g && res_in && res_out, "NULL argument");
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK((((uintptr_t)g | (uintptr_t)res_in | (uintptr_t)res_out) & 15) == 0,
           "g, res_in and res_out must be 16-byte aligned");
  FC_CHECK(!ef_overlap(res_out, g, n) && !ef_overlap(res_out, res_in, n),
           "res_out must not alias g or res_in");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t need = (n + 4ull * kBlock - 1) / (4ull * kBlock);
  const dim3 grid((uint32_t)std::min<uint64_t>(need, 256u * 16u));
  TimedLaunch t(FC_TIME_COMPACT, s);
  hipLaunchKernelGGL(k_ef_sum, grid, dim3(kBlock), 0, s, g, res_in, res_out, n);
  FC_LAUNCHED("k_ef_sum");
  return FC_OK;
}

int fc_ef_clear(const fc_packet_view* pkt, uint64_t n, float* res_out, fc_stream_t stream) {
  FC_CHECK(pkt && res_out, "NULL argument");
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(pkt->idx && pkt->val && pkt->cnt && pkt->hdr, "packet view incomplete (idx/val packet)");
  EfClearArgs a;
  memset(&a, 0, sizeof a);
  a.idx = (const uint16_t*)pkt->idx; a.val = pkt->val; a.cnt = pkt->cnt; a.hdr = pkt->hdr;
  a.out = res_out; a.n = n; a.ib = index_bits(n); a.nchunks = num_chunks(n);
  hipStream_t s = (hipStream_t)stream;
  TimedLaunch t(FC_TIME_DECODE, s);
  hipLaunchKernelGGL(k_ef_clear, dim3(decode_grid(n, 8)), dim3(kBlock), 0, s, a);
  FC_LAUNCHED("k_ef_clear");
  return FC_OK;
}

int fc_topk_encode_ef(const float* g, const float* res_in, float* res_out, uint64_t n, uint64_t k,
                      uint16_t* idx, float* val, uint64_t capacity, uint32_t* cnt, uint64_t* qoff,
                      fc_packet_hdr* hdr, void* ws, size_t ws_bytes, fc_stream_t stream) {
  FC_CHECK(res_in != nullptr && res_out != nullptr, "res_in / res_out is NULL");
  FC_CHECK((((uintptr_t)res_in | (uintptr_t)res_out) & 15) == 0,
           "res_in and res_out must be 16-byte aligned");
  FC_CHECK(k > 0 && k < n, "fc_topk_encode_ef needs 0 < k < n (k=%llu, n=%llu): trivial k is "
           "fc_ef_sum + fc_topk_encode_exact + fc_ef_clear", (unsigned long long)k,
           (unsigned long long)n);
  CompactArgs ca; EngineArgs ea; ResolveArgs ra; HdrInit hi;
  int rc = topk_args(g, n, k, FC_KEY_MAGNITUDE, 0, 0, idx, val, capacity, cnt, qoff, hdr, ws,
                     ws_bytes, &ca, &ea, &ra, &hi);
  if (rc) return rc;
  FC_CHECK(!ef_overlap(res_out, g, n) && !ef_overlap(res_out, res_in, n),
           "res_out must not alias g or res_in");
  hipStream_t s = (hipStream_t)stream;
  // fc_topk_encode's plan: the bracket, and so the packet's slack, is the one it would list for a
  const SamplePlan P = make_plan(n, k);
  const uint32_t sgrid = (P.nseg + P.segs - 1) / P.segs;
  {
    TimedLaunch t(FC_TIME_SAMPLE, s);
    hipLaunchKernelGGL(k_sample1_ef, dim3(sgrid), dim3(kBlock), 0, s, g, res_in, P, ca.W, ca.ib, hdr, hi);
    FC_LAUNCHED("k_sample1_ef");
  }
  {
    TimedLaunch t(FC_TIME_COMPACT, s);
    EfArgs ef;
    ef.res_in = res_in; ef.res_out = res_out;
    hipLaunchKernelGGL(k_compact_mag1_ef, dim3(ca.nchunks), dim3(kCBlock), 0, s, ca, ef);
    FC_LAUNCHED("k_compact_mag1_ef");
  }
  // k_resolve<true> bins the candidates; k_resolve<false, EF> gathers, finds T64 and zeroes the
  // selected candidates in res_out (ra.dense)
  ra.rbin = 1;
  ra.dense = res_out;
  const uint32_t want = std::max<uint32_t>(32u, std::min<uint32_t>((uint32_t)kResolveGrid,
                                            (ra.nchunks + FC_RESOLVE_CPW - 1) / FC_RESOLVE_CPW));
  const dim3 grid(resolve_grid(ra.nchunks, want));
  TimedLaunch t(FC_TIME_ENGINE, s);
  hipLaunchKernelGGL(k_resolve<true>, grid, dim3(kBlock), 0, s, ra);
  FC_LAUNCHED("k_resolve<bin>");
  hipLaunchKernelGGL((k_resolve<false, true>), grid, dim3(kBlock), 0, s, ra);
  FC_LAUNCHED("k_resolve<gather, ef>");
  return FC_OK;
}

int fc_topk_encode_ef_batch(const fc_encode_job* jobs, const fc_ef_job* ef, int m, uint64_t n,
                            uint64_t k, uint64_t capacity, void* ws, size_t ws_bytes,
                            fc_stream_t stream) {
  // fc_topk_encode_batch_part's checks (the tables are device memory: their contents are the
  // caller's contract)
  FC_CHECK(jobs != nullptr, "jobs is NULL");
  FC_CHECK(ef != nullptr, "ef jobs is NULL");
  FC_CHECK(m >= 1 && m <= 65535, "m=%d outside [1, 65535]", m);
  FC_CHECK(n >= 2 && n <= 0xffffffffull, "n=%llu outside [2, 2^32-1]", (unsigned long long)n);
  FC_CHECK(k > 0 && k < n, "batched error-feedback encode needs 0 < k < n (k=%llu): trivial k is "
           "fc_ef_sum + fc_topk_encode_exact + fc_ef_clear per client", (unsigned long long)k);
  FC_CHECK(capacity >= fc_packet_capacity(n), "capacity %llu < fc_packet_capacity(n) %llu",
           (unsigned long long)capacity, (unsigned long long)fc_packet_capacity(n));
  FC_CHECK(ws != nullptr, "workspace is NULL");
  if (ws_bytes < fc_workspace_bytes_batch(n, m))
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes,
                fc_workspace_bytes_batch(n, m));
  const uint32_t ib = index_bits(n);
  const uint64_t stride = WsLayout::of(n).bytes;
  HdrInit hi;
  memset(&hi, 0, sizeof hi);
  hi.n = (uint32_t)n; hi.k = (uint32_t)k; hi.ib = ib;
  hi.codec = FC_CODEC_TOP; hi.format = FC_FMT_IDXVAL; hi.key_mode = FC_KEY_MAGNITUDE;
  CompactArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.n = n; ca.ib = ib; ca.nchunks = num_chunks(n); ca.W = ws_ptrs(ws, n); ca.HI = hi;
  ca.jobs = jobs; ca.ws_stride = stride;
  ResolveArgs ra;
  memset(&ra, 0, sizeof ra);
  ra.ib = ib; ra.nchunks = ca.nchunks; ra.k = k; ra.key_mode = FC_KEY_MAGNITUDE;
  ra.W = ca.W; ra.jobs = jobs; ra.ws_stride = stride; ra.ef = ef;
  ra.rbin = 1;                       // k_resolve<true> bins the candidates
  hipStream_t s = (hipStream_t)stream;
  // fc_topk_encode_batch's plan (cbins_log2 and FC_SAMPLE_ROUNDS included): the same bracket,
  // and so the same slack entries, as it lists for a
  SamplePlan P = make_plan(n, k);
  P.cbins_log2 = cand_bins_log2(n, P);
  const dim3 sgrid((P.pstride + FC_SAMPLE_ROUNDS - 1) / FC_SAMPLE_ROUNDS, (uint32_t)m);
  {
    TimedLaunch t(FC_TIME_SAMPLE, s);
    hipLaunchKernelGGL(k_pilot_ef, dim3((uint32_t)m), dim3(kBlock), 0, s, P, ca.W, jobs, ef, stride);
    FC_LAUNCHED("k_pilot_ef");
    hipLaunchKernelGGL(k_sample1_ef_batch, sgrid, dim3(kBlock), 0, s, P, ca.W, ib, hi, jobs, ef, stride);
    FC_LAUNCHED("k_sample1_ef_batch");
  }
  {
    TimedLaunch t(FC_TIME_COMPACT, s);
    const dim3 grid = compact_mag_grid(ca, (uint32_t)m);
    hipLaunchKernelGGL(k_compact_mag1_ef_batch, grid, dim3(kCBlock), 0, s, ca, ef);
    FC_LAUNCHED("k_compact_mag1_ef_batch");
  }
  const dim3 rgrid(resolve_grid(ca.nchunks, kResolveGridBatch), (uint32_t)m);
  TimedLaunch t(FC_TIME_ENGINE, s);
  hipLaunchKernelGGL(k_resolve<true>, rgrid, dim3(kBlock), 0, s, ra);
  FC_LAUNCHED("k_resolve<bin>");
  hipLaunchKernelGGL((k_resolve<false, true>), rgrid, dim3(kBlock), 0, s, ra);
  FC_LAUNCHED("k_resolve<gather, ef>");
  return FC_OK;
}

}  // extern "C"
