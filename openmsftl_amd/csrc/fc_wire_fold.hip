// fc_wire_fold.hip — the FedAVG fold straight from wire packets for MI355X (gfx950): what
// fc_wire_unpack_batch into fresh packets followed by fc_decode_accumulate(_continue) gives, bit
// for bit, without the slotted packets in between.  Each packet's bytes are read once.
//
// k_fold_wire<ACC_IN> is k_fold_q (fc_decode.hip, whose comments record why each choice was made)
// on another base: one 256-thread workgroup per chunk, wave q owns quarter q (a 2048-float LDS
// tile) and folds every packet's entries of that quarter in row order,
//     tile[loc] = fl(tile[loc] + fl(v * w))            (__fmul_rn / __fadd_rn, no FMA)
// with no workgroup barrier after the prologue, no atomics on the result and no workgroup waiting
// for another.  Quarter q of chunk c of a wire packet is the range [st + b_q, st + b_q+1) of its
// compact idx / val sections (st = start[c], b = the chunk's quarter-offset word), where the
// slotted packet has [c * 8192 + b_q, c * 8192 + b_q+1).
//
// Memory safety, whatever the bytes hold (the argument of k_wire_unpack, restated):
//   * the header is read only when the host's byte length is >= 128; a buffer whose magic,
//     version, nch, n or E does not fit the caller's n and the byte length is a packet with no
//     entries, and nothing else of it is read;
//   * otherwise wire_layout(n, E).total <= bytes, so both tables and entries [0, E) of the idx and
//     val sections lie below the byte length; st = min(start, E), cnt = min(word >> 48, 8192,
//     E - st) and q1 <= q2 <= q3 <= cnt are clamped as there, so every entry read is below E;
//   * an item with no entries (its first entry may be E, its packet may be none) reads no byte
//     of the buffer: the fast body's unconditional loads take the first weight instead;
//   * every LDS location is masked into the quarter (lc & 2047) or compared against it
//     (loc < 2048); no address comes from the content unclamped.
// The keep rule is the decoders' (a validated payload may list an entry below thresh):
// the float form of comp >= T64 in the fast body, entry_kept per entry in the slow body.
//
// Included by fedcodec.hip after fc_decode.hip and fc_wire.hip (one translation unit).

namespace fc {

// The per-packet record in LDS: 32 bytes (k_fold_q's QMeta has 48; with the 32 KB tile the
// workgroup stays at four per CU).  The section pointers are derived from wire, n and E at the
// point of use; p, seed and offset are read from the header on the slow path only.
struct WMeta {
  const unsigned char* wire;                    // the 128-byte header; nullptr: no entries
  uint64_t thresh;
  uint32_t E;
  float w;
  uint32_t flags;                               // ib | codec << 8 | key_mode << 16 | poison << 24
  uint32_t pad_;
};
static_assert(sizeof(WMeta) <= 48, "k_fold_wire: four workgroups per CU");

struct WireFoldArgs {
  const fc_wire_job* jobs;                      // DEVICE array of m wire buffers and byte lengths
  const float* weights;                         // DEVICE fp32[m]
  float* out;
  uint64_t n;
  uint32_t m, nch;
  int acc_in;
};

// seed, offset and p of the slow body's rules, from the wire header (a packet with no entries:
// nothing is read and nothing of it is used)
__device__ __forceinline__ PktCache wire_pkt_cache(const WMeta& pm) {
  PktCache pk;
  const uint32_t fl = uni32(pm.flags);
  pk.thresh = uni64(pm.thresh); pk.ib = fl & 0xffu;
  pk.codec = (fl >> 8) & 0xffu; pk.key_mode = (fl >> 16) & 0xffu;
  pk.seed = 0; pk.offset = 0; pk.p = 0.0;
  const fc_wire_hdr* h = (const fc_wire_hdr*)uni_ptr(pm.wire);
  if (h != nullptr) { pk.seed = h->pkt.seed; pk.offset = h->pkt.offset; pk.p = h->pkt.p; }
  return pk;
}

template <bool ACC_IN>
__global__ __launch_bounds__(kQBlock, 4) void k_fold_wire(WireFoldArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kChunk];
  __shared__ WMeta s_meta[kSparseMaxM];
  __shared__ uint32_t s_mark[4][kQuarter / 32];   // poisoning packets: kept-location bits
  __shared__ uint32_t s_slow;
  const int tid = threadIdx.x, lane = lane_id();
  const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t M = a.m;
  const uint32_t c = blockIdx.x;
  const uint32_t base = c * (uint32_t)kChunk;     // n < 2^32
  const uint32_t qbase = base + (uint32_t)(q * kQuarter);
  // the sections' offsets but for val's, which depends on the packet's E
  const uint64_t off_start = kWireHdrBytes + wire_pad16(8ull * a.nch);
  const uint64_t off_idx = off_start + wire_pad16(4ull * a.nch);
  if (tid == 0) s_slow = 0;
  s_mark[q][lane] = 0u;
  __syncthreads();
  if (tid < (int)M) {
    const fc_wire_job job = a.jobs[tid];
    const unsigned char* wire = static_cast<const unsigned char*>(job.wire);
    WMeta d;
    // a buffer that is no packet of length n inside its bytes (k_wire_unpack's decision): what
    // the unpack makes of it, an empty top-k packet that selects nothing
    d.wire = nullptr; d.thresh = kSelectNothing; d.E = 0; d.w = a.weights[tid]; d.pad_ = 0;
    uint32_t ib = 1u, codec = FC_CODEC_TOP, key_mode = FC_KEY_MAGNITUDE;
    bool poison = false;
    if (wire != nullptr && job.bytes >= kWireHdrBytes) {
      const fc_wire_hdr* h = reinterpret_cast<const fc_wire_hdr*>(wire);
      const uint64_t E = h->n_entries;
      if (h->magic == kWireMagic && h->version == kWireVersion && h->nch == a.nch &&
          (uint64_t)h->pkt.n == a.n && E <= 0xffffffffull && wire_layout(a.n, E).total <= job.bytes) {
        d.wire = wire; d.thresh = h->pkt.thresh; d.E = (uint32_t)E;
        ib = h->pkt.index_bits & 0xffu; codec = h->pkt.codec; key_mode = h->pkt.key_mode;
        const float dz = (codec == FC_CODEC_DROPOUT_UNBIASED && h->pkt.p == 0.0) ? __uint_as_float(0x7fc00000u) : 0.0f;
        poison = __fmul_rn(dz, d.w) != __fmul_rn(dz, d.w);
      }
    }
    // the fast body's float form of comp >= T64 needs T64's key below +inf bits (see k_fold_q)
    const bool generic = codec == FC_CODEC_DROPOUT_UNBIASED || (key_mode == FC_KEY_PHILOX && d.thresh != 0) ||
                         (d.thresh >> ib) >= 0x7f800000ull;
    d.flags = ib | ((codec & 0xffu) << 8) | ((key_mode & 0xffu) << 16) | ((uint32_t)poison << 24);
    s_meta[tid] = d;
    if (poison || generic) atomicOr(&s_slow, 1u);
  }
  __syncthreads();                              // the only workgroup barriers
  const bool slow = s_slow != 0;
  // this chunk's table words of packets lane and lane + 64 (a per-lane pointer), clamped as
  // k_wire_unpack clamps them, and of them this wave's quarter: its first entry (absolute, <= E)
  // and its count (<= 8192)
  auto qload = [&](uint32_t m, uint32_t& first, uint32_t& count) {
    first = 0u; count = 0u;
    if (m >= M) return;
    const WMeta& pm = s_meta[m];
    const unsigned char* wire = pm.wire;
    if (wire == nullptr) return;
    const uint32_t E = pm.E;
    const uint64_t qo = ((wu64*)(wire + kWireHdrBytes))[c];
    const uint32_t st = min(((gu32*)(wire + off_start))[c], E);
    const uint32_t cnt = min(min((uint32_t)(qo >> 48), (uint32_t)kChunk), E - st);
    const uint32_t q3 = min((uint32_t)(qo >> 32) & 0xffffu, cnt);
    const uint32_t q2 = min((uint32_t)(qo >> 16) & 0xffffu, q3);
    const uint32_t q1 = min((uint32_t)qo & 0xffffu, q2);
    const uint32_t lo = q == 0 ? 0u : q == 1 ? q1 : q == 2 ? q2 : q3;
    const uint32_t hi = q == 0 ? q1 : q == 1 ? q2 : q == 2 ? q3 : cnt;
    first = st + lo; count = hi - lo;           // first + count <= st + cnt <= E
  };
  uint32_t f0, n0, f1, n1;
  qload((uint32_t)lane, f0, n0);
  qload((uint32_t)lane + 64u, f1, n1);
  // a quarter holding more than kQTail * 64 entries in any packet sends this wave to the slow body
  const bool dense_q = __any(n0 > (uint32_t)(kQTail * 64) || n1 > (uint32_t)(kQTail * 64));
  auto range = [&](uint32_t m, uint32_t& first, uint32_t& count) {   // uniform
    first = (uint32_t)__builtin_amdgcn_readlane((int)(m < 64 ? f0 : f1), (int)(m & 63));
    count = (uint32_t)__builtin_amdgcn_readlane((int)(m < 64 ? n0 : n1), (int)(m & 63));
  };
  // a packet's entry sections from its base and E (uniform); entry e < E is inside both
  auto sec_idx = [&](const WMeta& pm) -> gu16* {
    return (gu16*)(uni_ptr(pm.wire) + off_idx);
  };
  auto sec_val = [&](const WMeta& pm) -> gf32* {
    return (gf32*)(uni_ptr(pm.wire) + off_idx + wire_pad16(2ull * uni32(pm.E)));
  };
  // ---- tile init: +0 (np.sum's start) or the partial sum being continued ----
  float* qt = tile + q * kQuarter;
  bool nz = false;                                  // ACC_IN: the sum to continue holds a -0.0
#pragma unroll
  for (int i = 0; i < kQuarter / 256; ++i) {
    const uint32_t loc = (uint32_t)(i * 256 + lane * 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ACC_IN) {
      v = load4(a.out, (uint64_t)qbase + loc, a.n);
      nz = nz || __float_as_uint(v.x) == 0x80000000u || __float_as_uint(v.y) == 0x80000000u ||
           __float_as_uint(v.z) == 0x80000000u || __float_as_uint(v.w) == 0x80000000u;
    }
    *reinterpret_cast<float4*>(&qt[loc]) = v;
  }
  const bool neg0_in = ACC_IN && __any(nz);         // wave-uniform; never true for a sum a fold made
  if (slow || dense_q) {
    // ---- slow body (a launch holding rand-k Philox, dropout-unbiased or NaN-poisoning packets,
    // or a quarter with more than kQTail * 64 entries): item by item, every rule per entry ----
    for (uint32_t m = 0; m < M; ++m) {
      uint32_t first, count;
      range(m, first, count);
      const WMeta& pm = s_meta[m];
      const uint32_t fl = uni32(pm.flags);
      if (count == 0 && !((fl >> 24) & 1u)) continue;   // uniform: nothing to fold, nothing to poison
      const PktCache pk = wire_pkt_cache(pm);
      const float w = __uint_as_float(uni32(__float_as_uint(pm.w)));
      gu16* pidx = sec_idx(pm) + first;
      gf32* pval = sec_val(pm) + first;
      if ((fl >> 24) & 1u) {                        // poisoning: NaN where this packet folds nothing
        for (uint32_t e = lane; e < count; e += 64) {
          const uint32_t id = base + pidx[e];
          const uint32_t loc = id - qbase;
          if (loc < (uint32_t)kQuarter && entry_kept(pk, id, pval[e]))
            atomicOr(&s_mark[q][loc >> 5], 1u << (loc & 31));
        }
        const uint32_t bits = s_mark[q][lane];
        for (int b = 0; b < 32; ++b)
          if (!((bits >> b) & 1u)) qt[lane * 32 + b] = __uint_as_float(0x7fc00000u);
        s_mark[q][lane] = 0u;
      }
      for (uint32_t e = lane; e < count; e += 64)
        fold_q_entry<false>(pk, w, qt, qbase, base + pidx[e], pval[e]);
    }
  } else {
    // ---- fast body: top-k / mask-selected packets; k_fold_q's two register slots of kQGroup
    // items, the loads of one group in flight while the other is folded.  Per entry:
    // loc = lc & 2047, one count compare and comp >= T64 in float form,
    //     comp >= T64  <=>  !(|v| <= Tf)  ||  (|v| == Tf && lc >= Ti - chunk base).
    // Lanes past the item's end re-read its last entry and fold into a dummy slot.
    uint32_t ids_[2][kQGroup][kQR];
    float vs_[2][kQGroup][kQR];
    uint32_t qn_[2][kQGroup];                                   // the item's entries (uniform)
    auto issue = [&](int sl, uint32_t m0) {
#pragma unroll
      for (int d = 0; d < kQGroup; ++d) {
        const uint32_t m = min(m0 + (uint32_t)d, M - 1);          // past the end: re-load (ignored)
        uint32_t first, count;
        range(m, first, count);
        qn_[sl][d] = count;
        const WMeta& pm = s_meta[m];
        // the loads stay unconditional (a branch around them would make the compiler wait for
        // the other slot's loads too): an item with no entries, whose `first` may be E or whose
        // packet may be none at all, loads the first weight instead (ignored: lim <= 0)
        gf32* val = count ? sec_val(pm) + first : (gf32*)a.weights;
        gu16* idx = count ? sec_idx(pm) + first : (gu16*)a.weights;
        const uint32_t last = count ? count - 1u : 0u;
#pragma unroll
        for (int r = 0; r < kQR; ++r) {
          const uint32_t e = min((uint32_t)(lane + r * 64), last);
          vs_[sl][d][r] = val[e];
          ids_[sl][d][r] = idx[e];
        }
      }
    };
    auto process = [&](int sl, uint32_t m0) {
#pragma unroll
      for (int d = 0; d < kQGroup; ++d) {
        const uint32_t m = m0 + (uint32_t)d;
        if (m >= M) break;                                        // uniform
        const WMeta& pm = s_meta[m];
        const float w = __uint_as_float(uni32(__float_as_uint(pm.w)));
        const uint64_t thresh = uni64(pm.thresh);
        const uint32_t ib = uni32(pm.flags) & 0xffu;
        const float Tf = __uint_as_float((uint32_t)(thresh >> ib));
        const uint32_t Ti = (uint32_t)(thresh & ((1ull << ib) - 1ull));
        const uint32_t Tr = Ti <= base ? 0u : min(Ti - base, (uint32_t)kChunk);   // tie cut in the chunk
        const uint32_t qn = qn_[sl][d];
        const int lim = (int)qn - lane;                           // entries left for this lane
        float* slot[kQR];
        float tv[kQR];
        float* dummy = reinterpret_cast<float*>(&s_mark[q][lane]);
#pragma unroll
        for (int r = 0; r < kQR; ++r) {                           // all tile reads, then writes
          const uint32_t lc = ids_[sl][d][r];                     // chunk-local
          const float v = vs_[sl][d][r];
          const float av = __builtin_fabsf(v);
          const bool ok = (lim > r * 64) & (!(av <= Tf) | ((av == Tf) & (lc >= Tr)));
          slot[r] = ok ? qt + (lc & (uint32_t)(kQuarter - 1)) : dummy;
          tv[r] = *slot[r];
        }
#pragma unroll
        for (int r = 0; r < kQR; ++r)
          *slot[r] = __fadd_rn(tv[r], __fmul_rn(vs_[sl][d][r], w));
        if (kQTail > kQR && qn > (uint32_t)(kQR * 64)) {          // rare, uniform: the rest
          uint32_t first, count;
          range(m, first, count);
          gf32* val = sec_val(pm) + first;
          gu16* idx = sec_idx(pm) + first;
          for (uint32_t e = (uint32_t)(kQR * 64) + lane; e < count; e += 64) {
            const uint32_t lc = idx[e];
            const float v = val[e];
            const float av = __builtin_fabsf(v);
            const uint32_t l2 = lc & (uint32_t)(kQuarter - 1);
            if (!(av <= Tf) | ((av == Tf) & (lc >= Tr)))
              qt[l2] = __fadd_rn(qt[l2], __fmul_rn(v, w));
          }
        }
      }
    };
    issue(0, 0);
    for (uint32_t m0 = 0; m0 < M; m0 += 2 * kQGroup) {
      issue(1, m0 + kQGroup);
      process(0, m0);
      if (m0 + kQGroup >= M) break;                                // uniform
      issue(0, m0 + 2 * kQGroup);
      process(1, m0 + kQGroup);
    }
  }
  if (neg0_in) {
    // ---- the continued sum held -0.0 (k_fold_q's fix-up, restated): a coordinate that is still
    // -0.0 here has been -0.0 all along, and the dense sum leaves it -0.0 only if every packet
    // with a sign-positive weight kept it: mark what each such packet keeps and turn the unmarked
    // -0.0 into +0 ----
    for (uint32_t m = 0; m < M; ++m) {
      const WMeta& pm = s_meta[m];
      const float w = __uint_as_float(uni32(__float_as_uint(pm.w)));
      if (__float_as_uint(w) >> 31) continue;       // fl(+0 * w) = -0: skipping it was exact
      uint32_t first, count;
      range(m, first, count);
      const PktCache pk = wire_pkt_cache(pm);
      s_mark[q][lane] = 0u;                         // (the fast body's dummy slots)
      if (count != 0) {                             // uniform
        gu16* pidx = sec_idx(pm) + first;
        gf32* pval = sec_val(pm) + first;
        for (uint32_t e = lane; e < count; e += 64) {
          const uint32_t id = base + pidx[e];
          const uint32_t loc = id - qbase;
          if (loc < (uint32_t)kQuarter && entry_kept(pk, id, pval[e]))
            atomicOr(&s_mark[q][loc >> 5], 1u << (loc & 31));
        }
      }
      const uint32_t bits = s_mark[q][lane];
      for (int b = 0; b < 32; ++b)
        if (!((bits >> b) & 1u) && __float_as_uint(qt[lane * 32 + b]) == 0x80000000u)
          qt[lane * 32 + b] = 0.0f;
      s_mark[q][lane] = 0u;
    }
  }
  // ---- write the quarter out ----
#pragma unroll
  for (int i = 0; i < kQuarter / 256; ++i) {
    const uint32_t loc = (uint32_t)(i * 256 + lane * 4);
    store_out(a.out, (uint64_t)qbase + loc, a.n, *reinterpret_cast<const float4*>(&qt[loc]));
  }
}

template __global__ void k_fold_wire<false>(WireFoldArgs);
template __global__ void k_fold_wire<true>(WireFoldArgs);

}  // namespace fc

extern "C" {

int fc_wire_fold(const fc_wire_job* jobs_dev, const float* weights_dev, int m, uint64_t n,
                 float* acc, int continue_sum, fc_stream_t stream) {
  FC_CHECK(jobs_dev != nullptr, "jobs_dev is NULL");
  FC_CHECK(weights_dev != nullptr, "weights_dev is NULL");
  FC_CHECK(acc != nullptr, "acc is NULL");
  FC_CHECK(m >= 1 && m <= 65535, "m=%d outside [1, 65535]", m);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)acc & 15) == 0, "acc must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // <= kSparseMaxM packets per launch; later launches continue the same left-to-right sum
  for (int m0 = 0; m0 < m; m0 += kSparseMaxM) {
    WireFoldArgs a;
    memset(&a, 0, sizeof a);
    a.jobs = jobs_dev + m0; a.weights = weights_dev + m0; a.out = acc; a.n = n;
    a.m = (uint32_t)std::min(m - m0, (int)kSparseMaxM); a.nch = num_chunks(n);
    a.acc_in = continue_sum != 0 || m0 > 0;
    if (a.acc_in) hipLaunchKernelGGL(k_fold_wire<true>, dim3(a.nch), dim3(kQBlock), 0, s, a);
    else hipLaunchKernelGGL(k_fold_wire<false>, dim3(a.nch), dim3(kQBlock), 0, s, a);
    FC_LAUNCHED("k_fold_wire");
  }
  return FC_OK;
}

}  // extern "C"
