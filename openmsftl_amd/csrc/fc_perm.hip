// fc_perm.hip — np.random.permutation(n)[:k] of NumPy's legacy MT19937 stream on the device.
//
// The reference's 'rand' codec keeps the coordinates np.random.permutation(n)[:k]
// (ftl/compression/compression.py:43-44).  NumPy shuffles arange(n) from the top:
//   for i = n-1 down to 1:  j = random_interval(i);  swap x[i], x[j]
// and random_interval(i) draws 32-bit outputs w until (w & mask(i)) <= i, mask(i) the smallest
// 2^b - 1 >= i.  One call here reproduces idx = x[:k] (order included), the index set as bit
// words, and the state np.random is left in, from a state block that lives on the device and is
// updated in place, so consecutive rows chain without the host:
//   1 words   the tempered outputs from the state block's (key, pos), cut into segments of
//             kSegW words: one wave per segment jumps to its start (fc::mt::jump_wave over the
//             raw sequence of the key; the polynomials z^(s kSegW - 1) do not depend on n) and
//             twists its own 624-word window in LDS, as k_mt_binom does;
//   2 parse   which word belongs to which step: word q is tested against i = n-1-A(q), A(q) the
//             number of accepted words before q.  One wave walks the words in order, 128 at a
//             time (two per lane): every word is tested against the group's first i; its true
//             step is i - p0, p0 <= 127 the number of accepted words before it in the group, so
//             the group is exact as it stands when no accepted word has (w & mask) > i - 127
//             and the mask does not change inside the group (induction over the words);
//             otherwise the group is resolved word by word.  The accepted word of step i gives j_i = w & mask(i),
//             written to J[n-1-i] (draw order).  The other waves of the workgroup stage the
//             words in LDS a chunk ahead of the walk;
//   3 link    per-position lists of the steps i with j_i == c (head[c] / next[i], atomic
//             exchange; the trace takes minima, so the list order does not matter);
//   4 trace   for p < k, backwards in time from the last step (i = 1) to the first (i = n-1):
//             position c, time t; the smallest step i > t that touched c is step c itself
//             (c > t: the content came from j_c) or the smallest list entry above t (the content
//             came from position i); the walk ends at the position whose initial content,
//             x0[c] = c, is the answer;
//   5 state   after c words from raw offset pos the key is block b = (pos + c - 1) / 624 of the
//             raw sequence and pos' = pos + c - 624 b (NumPy twists lazily): the block's words
//             are the untempered outputs 624 b - pos .. + 624 of stage 1.
// Every loop is bounded: a parse that runs out of its word budget sets the state block's
// fallback word to 1, a trace that reaches its bounds sets it to 2; the remaining kernels of
// the call then return at once, key and pos stay as they were, and later calls on the block
// draw nothing (the caller makes NumPy's own call on the host from that state).  Stages are
// separate launches in stream order; nothing waits inside a kernel and the host never waits.

namespace fc {
namespace perm {

using mt::kN;
using mt::kPolyWords;
using mt::kRaw;
using mt::kRawLds;
using mt::kWg;

constexpr uint32_t kSegW = 2 * mt::kSeg;            // words per generator wave
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kU = 8;                          // word groups the parse holds in registers
constexpr uint32_t kGroupW = 128;                   // words per group of the parse: two per lane
constexpr uint32_t kChunkW = 16384;                 // words per LDS half of the parse (divides kSegW)
constexpr uint32_t kParseThreads = 320;             // the parsing wave + four copying waves
constexpr uint32_t kParseLds = (2 * kChunkW + 64) * 4;
constexpr uint32_t kTraceRounds = 4096;             // bound of a trace (expected: ~ln n rounds)
constexpr uint32_t kListBound = 4096;               // bound of one list walk (expected: ~ln(n/c))

struct PermState {                                  // = fc_perm_state (include/fedcodec.h)
  uint32_t key[kN];
  uint32_t pos, fallback, rows_done, reserved;
  uint64_t consumed;
};

struct PermHdr {                                    // workspace offset 0: the call's pending state
  uint32_t newkey[kN];
  uint32_t newpos, key_changed;
  uint64_t consumed;
};

__device__ __forceinline__ uint32_t untemper(uint32_t y) {
  y ^= y >> 18;
  y ^= (y << 15) & 0xefc60000u;
  uint32_t t = y;
#pragma unroll
  for (int r = 0; r < 5; ++r) t = y ^ ((t << 7) & 0x9d2c5680u);
  y = t;
#pragma unroll
  for (int r = 0; r < 3; ++r) t = y ^ (t >> 11);
  return t;
}

__global__ void __launch_bounds__(64) k_perm_begin(PermState* st, mt::Words624 w, uint32_t pos) {
  for (uint32_t j = threadIdx.x; j < kN; j += 64) st->key[j] = w.w[j];
  if (threadIdx.x == 0) {
    st->pos = pos;
    st->fallback = 0;
    st->rows_done = 0;
    st->reserved = 0;
    st->consumed = 0;
  }
}

// n <= 1: nothing is drawn; x = [0] (or empty).
__global__ void __launch_bounds__(64) k_perm_trivial(PermState* st, uint32_t* idx, uint32_t* mask,
                                                    uint32_t n, uint32_t k) {
  if (threadIdx.x != 0 || st->fallback) return;
  if (n == 1 && mask) mask[0] = k;
  if (k == 1 && idx) idx[0] = 0;
  st->rows_done += 1;
}

// Stage 1: words[s kSegW .. (s + 1) kSegW) = the outputs s kSegW .. of the state (key, pos);
// raw = the raw sequence of key (k_mt_raw).  Workgroup = kWg segments sharing one LDS copy.
__global__ void __launch_bounds__(64 * kWg) k_perm_words(const PermState* st,
                                                        const uint32_t* __restrict__ raw,
                                                        const uint32_t* __restrict__ polys,
                                                        uint32_t* __restrict__ words, uint32_t segs) {
  extern __shared__ uint32_t xs[];                     // kRawLds raw words, then kWg windows
  if (st->fallback) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t seg = blockIdx.x * kWg + wave;
  uint32_t* a = xs + kRawLds + wave * kN;
  const uint32_t pos = __builtin_amdgcn_readfirstlane(st->pos);
  mt::load_raw(xs, raw);
  __syncthreads();
  if (seg < segs) {
    if (seg == 0) {
      for (uint32_t j = lane; j < kN; j += 64) a[j] = xs[pos + j];
    } else {
      mt::jump_wave(xs, pos, polys + (uint64_t)seg * kPolyWords, a, lane);
    }
  }
  __syncthreads();
  if (seg >= segs) return;
  uint32_t* dst = words + (uint64_t)seg * kSegW;
  for (uint32_t done = 0; done < kSegW; done += kN) {
    if (done) mt::twist_wave(a, lane);
    for (uint32_t j = lane; j < kN && done + j < kSegW; j += 64) dst[done + j] = mt::temper(a[j]);
  }
}

struct ParseArgs {
  PermState* st;
  PermHdr* hd;
  const uint32_t* words;
  uint32_t* J;              // J[n - 1 - i] = j_i, i in [1, n): draw order, so that the
                            // stores of one group ascend with the lane (they coalesce)
  uint64_t limit;           // the word budget
  uint64_t cap;             // words generated (>= limit + 624)
  uint32_t n;
};

// The parse's workgroup barrier: LDS traffic only.  (__syncthreads would also wait for the
// parsing wave's stores to J, a memory round trip per chunk.)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Stage 2 (+ the pending state of stage 5), one workgroup: wave 0 parses chunk c from one half
// of LDS while the other waves copy chunk c + 1 into the other half (the walk is far shorter
// than a memory round trip per group, so the words have to be at hand).
__global__ void __launch_bounds__(kParseThreads) k_perm_parse(ParseArgs A) {
  extern __shared__ uint32_t xs[];                     // two chunks, then the stop word
  volatile uint32_t* s_stop = xs + 2 * kChunkW;
  if (A.st->fallback) return;
  const uint32_t lane = threadIdx.x & 63;
  // wave-uniform, and known to be: i and the walk's branches stay scalar
  const bool parser = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  const uint32_t* __restrict__ W = A.words;
  // every chunk below lies inside the generated words: cap is a multiple of kChunkW >= limit
  const uint32_t nchunks = (uint32_t)((A.limit + kChunkW - 1) / kChunkW);
  const uint32_t lt = threadIdx.x - 64;                // loader thread
  constexpr uint32_t kLoaders = kParseThreads - 64, kV = kChunkW / 4 / kLoaders;
  static_assert(kV * kLoaders * 4 == kChunkW, "the copying waves cover a chunk exactly");
  auto load_chunk = [&](uint32_t c) {
    const uint4* src = reinterpret_cast<const uint4*>(W + (uint64_t)c * kChunkW);
    uint4* dst = reinterpret_cast<uint4*>(xs + (c & 1) * kChunkW);
    uint4 r[kV];
#pragma unroll
    for (uint32_t v = 0; v < kV; ++v) r[v] = src[lt + v * kLoaders];
#pragma unroll
    for (uint32_t v = 0; v < kV; ++v) dst[lt + v * kLoaders] = r[v];
  };
  if (threadIdx.x == 0) *s_stop = 0;
  if (!parser) load_chunk(0);
  lds_barrier();
  uint32_t i = A.n - 1;                                // the step the next word is tested against
  uint64_t consumed = 0;
  bool done = false, out = false;
  for (uint32_t c = 0; c < nchunks; ++c) {
    if (!parser) {
      if (c + 1 < nchunks) load_chunk(c + 1);
    } else {
      const uint2* b = reinterpret_cast<const uint2*>(xs + (c & 1) * kChunkW);
      const bool whole = (uint64_t)(c + 1) * kChunkW <= A.limit;   // no budget test per group
      uint2 cur[kU], nxt[kU];
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) cur[u] = b[u * 64 + lane];
      for (uint32_t g0 = 0; g0 < kChunkW / kGroupW && !done && !out; g0 += kU) {
        if (g0 + kU < kChunkW / kGroupW) {
#pragma unroll
          for (uint32_t u = 0; u < kU; ++u) nxt[u] = b[(g0 + kU + u) * 64 + lane];
        }
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
          if (done || out) break;
          // a group: kGroupW = 128 words, lane l holds words 2l and 2l + 1 of it
          const uint64_t qg = (uint64_t)c * kChunkW + (g0 + u) * kGroupW;
          const uint32_t M = 0xffffffffu >> __builtin_clz(i);
          const uint32_t m0 = cur[u].x & M, m1 = cur[u].y & M;
          const bool a0 = m0 <= i, a1 = m1 <= i;
          // an accepting word is tested against i - (accepting words before it) >= i - 127:
          // near the threshold iff i - m < 127 (unsigned: a rejected m > i wraps far above)
          const bool amb = i - m0 < kGroupW - 1 || i - m1 < kGroupW - 1;
          const uint64_t acc0 = __ballot(a0), acc1 = __ballot(a1);
          const uint32_t cnt = (uint32_t)(__builtin_popcountll(acc0) + __builtin_popcountll(acc1));
          if (__ballot(amb) == 0 && i >= cnt + (M >> 1) + 1 && (whole || qg + kGroupW <= A.limit)) {
            uint32_t p0 = __builtin_amdgcn_mbcnt_hi(
                (uint32_t)(acc0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)acc0, 0u));
            p0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(acc1 >> 32),
                                           __builtin_amdgcn_mbcnt_lo((uint32_t)acc1, p0));
            uint32_t* dst = A.J + (A.n - 1 - i);       // one mask, no word near the threshold
            if (a0) dst[p0] = m0;
            if (a1) dst[p0 + a0] = m1;
            i = __builtin_amdgcn_readfirstlane(i - cnt);
          } else {
            for (uint32_t l = 0; l < kGroupW; ++l) {   // in order
              if (qg + l >= A.limit) { out = true; break; }
              const uint32_t wl = (l & 1) ? __builtin_amdgcn_readlane(cur[u].y, l >> 1)
                                          : __builtin_amdgcn_readlane(cur[u].x, l >> 1);
              const uint32_t ml = wl & (0xffffffffu >> __builtin_clz(i));
              if (ml <= i) {
                if (lane == 0) A.J[A.n - 1 - i] = ml;
                i = __builtin_amdgcn_readfirstlane(i - 1);
                if (i == 0) { consumed = qg + l + 1; done = true; break; }
              }
            }
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) cur[u] = nxt[u];
      }
      if ((done || out) && lane == 0) *s_stop = 1;
    }
    lds_barrier();
    if (__builtin_amdgcn_readfirstlane(*s_stop)) break;   // every wave reads the same word
    lds_barrier();                                     // ... before wave 0 may write it again
  }
  if (!parser) return;
  if (!done) {                                         // the budget ran out
    if (lane == 0) A.st->fallback = 1;
    return;
  }
  const uint32_t pos = A.st->pos;
  const uint64_t end = pos + consumed;                 // raw index of the next output
  const uint64_t b = (end - 1) / kN;
  if (b > 0) {
    const uint64_t q0 = b * kN - pos;                  // q0 + 623 <= consumed + 622 < cap
    for (uint32_t j = lane; j < kN; j += 64) A.hd->newkey[j] = untemper(W[q0 + j]);
  }
  if (lane == 0) {
    A.hd->newpos = (uint32_t)(end - b * kN);
    A.hd->key_changed = b > 0;
    A.hd->consumed = consumed;
  }
}

// Stage 3: next[i] = exchange(head[j_i], i) for every step that moves something.
__global__ void __launch_bounds__(256) k_perm_link(const PermState* st, const uint32_t* __restrict__ J,
                                                  uint32_t* head, uint32_t* next, uint32_t n) {
  if (st->fallback) return;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = 1 + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const uint32_t c = J[n - 1 - i];
    if (c != (uint32_t)i) next[i] = atomicExch(&head[c], (uint32_t)i);
  }
}

// Stage 4: idx[p] = x[p] after the shuffle, p < k; bit x[p] of mask.
__global__ void __launch_bounds__(256) k_perm_trace(PermState* st, const uint32_t* __restrict__ J,
                                                   const uint32_t* __restrict__ head,
                                                   const uint32_t* __restrict__ next, uint32_t n,
                                                   uint32_t k, uint32_t* idx, uint32_t* mask) {
  if (st->fallback) return;
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= k) return;
  uint32_t c = p, t = 0;
  if (c > 0) { t = c; c = J[n - 1 - c]; }              // step c is the last one to touch c
  bool over = true;
  for (uint32_t r = 0; r < kTraceRounds; ++r) {
    uint32_t best = kNone, e = head[c];
    for (uint32_t walked = 0; e != kNone && walked < kListBound; ++walked) {
      if (e > t && e < best) best = e;
      e = next[e];
    }
    if (e != kNone) break;
    if (best == kNone) { over = false; break; }
    c = t = best;
  }
  if (over) { st->fallback = 2; return; }
  if (idx) idx[p] = c;
  if (mask) atomicOr(&mask[c >> 5], 1u << (c & 31));
}

// Stage 5: the call's state becomes the block's, unless some stage fell back.
__global__ void __launch_bounds__(64) k_perm_commit(PermState* st, const PermHdr* hd) {
  if (st->fallback) return;
  if (hd->key_changed)
    for (uint32_t j = threadIdx.x; j < kN; j += 64) st->key[j] = hd->newkey[j];
  if (threadIdx.x == 0) {
    st->pos = hd->newpos;
    st->rows_done += 1;
    st->consumed += hd->consumed;
  }
}

}  // namespace perm
}  // namespace fc

// ---- host: segment polynomials, C ABI (include/fedcodec.h) ------------------------------------
#ifndef __HIP_DEVICE_COMPILE__
namespace fc {
namespace permhost {

constexpr uint64_t kMaxN = 0x7fffffffull;
static uint64_t budget(uint64_t n) { return 2 * n + 4096; }
static uint32_t segs_for(uint64_t words) {              // + 624: the key block may end past them
  return (uint32_t)((words + fc::mt::kN + fc::perm::kSegW - 1) / fc::perm::kSegW);
}

// polys[s] = z^(s kSegW - 1), s >= 1 (index 0 unused); grown on demand under g_mt_mu.
static std::vector<mthost::Poly> g_polys;
static const std::vector<mthost::Poly>& polys(uint32_t segs) {
  const mthost::Field* F = mthost::field();
  if (g_polys.empty()) {
    g_polys.resize(1);
    memset(&g_polys[0], 0, sizeof(mthost::Poly));
  }
  if (g_polys.size() < segs) {
    static const mthost::Poly zseg = F->powz(fc::perm::kSegW);
    while (g_polys.size() < segs) {
      mthost::Poly nx;
      if (g_polys.size() == 1) {
        nx = zseg;
        F->mulzinv(&nx);
      } else {
        F->mulmod(g_polys.back(), zseg, &nx);
      }
      g_polys.push_back(nx);
    }
  }
  return g_polys;
}

// Event pairs around the stages of the next calls (tools/perm_probe.py): off by default.
constexpr int kStages = 5;
static bool g_ptime = false;
static hipEvent_t g_pev[kStages + 1];
static bool g_pev_made = false, g_pev_rec = false;

}  // namespace permhost
}  // namespace fc

namespace {
constexpr size_t kPermPlanHdr = 256;
constexpr size_t kPermOffRaw = 2560;
constexpr size_t kPermOffJ = kPermOffRaw + (((size_t)fc::mt::kRaw * 4 + 255) & ~(size_t)255);
size_t perm_j_bytes(uint64_t n) { return ((size_t)n * 4 + 255) & ~(size_t)255; }
size_t perm_lds_words() { return ((size_t)fc::mt::kRawLds + (size_t)fc::mt::kWg * fc::mt::kN) * 4; }
int perm_lds_setup() {
  static int rc = hipFuncSetAttribute((const void*)fc::perm::k_perm_words,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)perm_lds_words()) == hipSuccess &&
                  hipFuncSetAttribute((const void*)fc::perm::k_perm_parse,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)fc::perm::kParseLds) == hipSuccess ? 0 : -1;
  return rc;
}
void perm_mark(int stage, hipStream_t s) {
  using namespace fc::permhost;
  if (!g_ptime) return;
  if (!g_pev_made) {
    for (auto& e : g_pev)
      if (hipEventCreate(&e) != hipSuccess) return;
    g_pev_made = true;
  }
  if (hipEventRecord(g_pev[stage], s) == hipSuccess && stage == kStages) g_pev_rec = true;
}
}  // namespace

static_assert(sizeof(fc::perm::PermState) == sizeof(fc_perm_state), "fc_perm_state layout");
static_assert(sizeof(fc::perm::PermHdr) <= kPermOffRaw, "PermHdr fits its slot");

extern "C" {

size_t fc_mt_perm_plan_bytes(uint64_t n) {
  if (n > fc::permhost::kMaxN) return 0;
  return kPermPlanHdr + (size_t)fc::permhost::segs_for(fc::permhost::budget(n)) * kMtPolyBytes;
}

size_t fc_mt_perm_workspace_bytes(uint64_t n) {
  if (n > fc::permhost::kMaxN) return 0;
  return kPermOffJ + perm_j_bytes(n) +
         (size_t)fc::permhost::segs_for(fc::permhost::budget(n)) * fc::perm::kSegW * 4;
}

int fc_mt_perm_plan(uint64_t n, void* plan, size_t plan_bytes, fc_stream_t stream) {
  FC_CHECK(n <= fc::permhost::kMaxN, "n=%llu outside [0, 2^31)", (unsigned long long)n);
  FC_CHECK(plan != nullptr, "plan is NULL");
  const size_t need = fc_mt_perm_plan_bytes(n);
  if (plan_bytes < need)
    return fail(FC_ERR_WORKSPACE, "plan %zu B < %zu B needed", plan_bytes, need);
  const uint32_t segs = fc::permhost::segs_for(fc::permhost::budget(n));
  std::vector<uint32_t> host(need / 4, 0);
  host[0] = (uint32_t)n;
  host[1] = segs;
  if (n >= 2) {
    std::lock_guard<std::mutex> g(fc::mthost::g_mt_mu);
    if (!(fc::mthost::field()->chi[fc::mthost::kD >> 6] >> (fc::mthost::kD & 63) & 1))
      return fail(FC_ERR_HIP, "MT19937 characteristic polynomial not found");
    const auto& P = fc::permhost::polys(segs);
    uint32_t* dst = host.data() + kPermPlanHdr / 4;
    for (uint32_t s = 1; s < segs; ++s) memcpy(dst + (size_t)s * kPolyWords, P[s].w, kMtPolyBytes);
  }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(plan, host.data(), need, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(FC_ERR_HIP, "fc_mt_perm_plan: copy failed");
  return FC_OK;
}

int fc_mt_perm_begin(const uint32_t* key, uint32_t pos, void* state, fc_stream_t stream) {
  FC_CHECK(key && state, "key and state must be non-NULL");
  FC_CHECK(pos <= kN, "pos=%u > 624", pos);
  fc::mt::Words624 kw;
  memcpy(kw.w, key, sizeof kw.w);
  hipLaunchKernelGGL(fc::perm::k_perm_begin, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     static_cast<fc::perm::PermState*>(state), kw, pos);
  FC_LAUNCHED("k_perm_begin");
  return FC_OK;
}

int fc_mt_permutation(const void* plan, size_t plan_bytes, uint64_t n, uint64_t k, uint64_t max_words,
                      void* state, uint32_t* idx_out, uint32_t* mask_bits, void* ws, size_t ws_bytes,
                      fc_stream_t stream) {
  FC_CHECK(n <= fc::permhost::kMaxN, "n=%llu outside [0, 2^31)", (unsigned long long)n);
  FC_CHECK(k <= n, "k=%llu > n=%llu", (unsigned long long)k, (unsigned long long)n);
  FC_CHECK(plan && state && ws, "plan, state and ws must be non-NULL");
  FC_CHECK(idx_out || mask_bits, "idx_out and mask_bits are both NULL");
  FC_CHECK(((uintptr_t)ws & 255) == 0, "ws must be 256-byte aligned");
  if (plan_bytes < fc_mt_perm_plan_bytes(n))
    return fail(FC_ERR_WORKSPACE, "plan %zu B < %zu B needed", plan_bytes, fc_mt_perm_plan_bytes(n));
  if (ws_bytes < fc_mt_perm_workspace_bytes(n))
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes,
                fc_mt_perm_workspace_bytes(n));
  hipStream_t s = (hipStream_t)stream;
  auto* st = static_cast<fc::perm::PermState*>(state);
  if (n <= 1) {
    hipLaunchKernelGGL(fc::perm::k_perm_trivial, dim3(1), dim3(64), 0, s, st, idx_out, mask_bits,
                       (uint32_t)n, (uint32_t)k);
    FC_LAUNCHED("k_perm_trivial");
    return FC_OK;
  }
  if (perm_lds_setup()) return fail(FC_ERR_HIP, "fc_mt_permutation: LDS attribute");
  // a budget above the default is cut to it: the workspace is sized for the default
  const uint64_t limit = max_words == 0 || max_words > fc::permhost::budget(n) ? fc::permhost::budget(n)
                                                                               : max_words;
  const uint32_t segs = fc::permhost::segs_for(limit);
  char* W = static_cast<char*>(ws);
  auto* hd = reinterpret_cast<fc::perm::PermHdr*>(W);
  uint32_t* raw = reinterpret_cast<uint32_t*>(W + kPermOffRaw);
  uint32_t* J = reinterpret_cast<uint32_t*>(W + kPermOffJ);
  uint32_t* words = reinterpret_cast<uint32_t*>(W + kPermOffJ + perm_j_bytes(n));
  uint32_t* head = words;                  // the words are dead once parsed: 2n + 4096 >= 2n
  uint32_t* next = words + n;
  const uint32_t* polys =
      reinterpret_cast<const uint32_t*>(static_cast<const char*>(plan) + kPermPlanHdr);
  perm_mark(0, s);
  hipLaunchKernelGGL(fc::mt::k_mt_raw, dim3(1), dim3(64), 0, s, st->key, (uint64_t)0, raw, (uint64_t)0);
  FC_LAUNCHED("k_mt_raw");
  hipLaunchKernelGGL(fc::perm::k_perm_words, dim3((segs + fc::mt::kWg - 1) / fc::mt::kWg),
                     dim3(64 * fc::mt::kWg), perm_lds_words(), s, st, raw, polys, words, segs);
  FC_LAUNCHED("k_perm_words");
  perm_mark(1, s);
  fc::perm::ParseArgs A;
  A.st = st;
  A.hd = hd;
  A.words = words;
  A.J = J;
  A.limit = limit;
  A.cap = (uint64_t)segs * fc::perm::kSegW;
  A.n = (uint32_t)n;
  hipLaunchKernelGGL(fc::perm::k_perm_parse, dim3(1), dim3(fc::perm::kParseThreads),
                     fc::perm::kParseLds, s, A);
  FC_LAUNCHED("k_perm_parse");
  perm_mark(2, s);
  if (mask_bits &&
      hipMemsetAsync(mask_bits, 0, (size_t)((n + 31) / 32) * 4, s) != hipSuccess)
    return fail(FC_ERR_HIP, "fc_mt_permutation: hipMemsetAsync");
  if (k > 0) {
    if (hipMemsetAsync(head, 0xff, (size_t)n * 4, s) != hipSuccess)
      return fail(FC_ERR_HIP, "fc_mt_permutation: hipMemsetAsync");
    const uint32_t lb = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16);
    hipLaunchKernelGGL(fc::perm::k_perm_link, dim3(lb), dim3(256), 0, s, st, J, head, next, (uint32_t)n);
    FC_LAUNCHED("k_perm_link");
    perm_mark(3, s);
    hipLaunchKernelGGL(fc::perm::k_perm_trace, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, s, st,
                       J, head, next, (uint32_t)n, (uint32_t)k, idx_out, mask_bits);
    FC_LAUNCHED("k_perm_trace");
  } else {
    perm_mark(3, s);
  }
  perm_mark(4, s);
  hipLaunchKernelGGL(fc::perm::k_perm_commit, dim3(1), dim3(64), 0, s, st, hd);
  FC_LAUNCHED("k_perm_commit");
  perm_mark(5, s);
  return FC_OK;
}

int fc_mt_perm_timing(int on, double* stage_ms) {
  using namespace fc::permhost;
  if (stage_ms) {
    FC_CHECK(g_pev_rec, "no timed fc_mt_permutation call to read");
    if (hipEventSynchronize(g_pev[kStages]) != hipSuccess)
      return fail(FC_ERR_HIP, "fc_mt_perm_timing: hipEventSynchronize");
    for (int i = 0; i < kStages; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, g_pev[i], g_pev[i + 1]) != hipSuccess)
        return fail(FC_ERR_HIP, "fc_mt_perm_timing: hipEventElapsedTime");
      stage_ms[i] = ms;
    }
  }
  g_ptime = on != 0;
  return FC_OK;
}

}  // extern "C"
#endif  // !__HIP_DEVICE_COMPILE__
