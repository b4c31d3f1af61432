// fc_wire_fold.hip — the FedAVG fold straight from wire packets for MI355X (gfx950): what
// fc_wire_unpack_batch into fresh packets followed by fc_decode_accumulate(_continue) gives, bit
// for bit, without the slotted packets in between.  Each packet's bytes are read once.
//
// k_fold_wire<ACC_IN> is fold_body (fc_decode.hip: the one body of the fold, with every tuning
// constant and the reason for it) on the source FoldWire below: quarter q of chunk c is the range
// [st + b_q, st + b_q+1) of the compact idx / val sections (st = start[c], b = qoff[c]).
//
// Memory safety, whatever the bytes hold:
//   * the header is read only when the host's byte length is >= 128; a buffer that wire_accept
//     (fc_wire_host.h, the rule k_wire_unpack applies) refuses is a packet with no entries, and
//     nothing else of it is read;
//   * otherwise both tables and entries [0, E) of idx and val lie below the byte length, and
//     wire_clamp (same header) gives st + cnt <= E, cnt <= 8192 and q1 <= q2 <= q3 <= cnt;
//   * an item with no entries (its first entry may be E, its packet may be none) reads no byte
//     of the buffer: the fast body's unconditional loads take the first weight instead;
//   * every LDS location is masked into the quarter (lc & 2047) or compared against it
//     (loc < 2048); no address comes from the content unclamped.
// (fedcodec.hip includes this file after fc_decode.hip and fc_wire.hip: one translation unit.)

namespace fc {

// The per-packet record in LDS: 32 bytes (QMeta: 48); sections, p, seed, offset are derived on use.
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

// fold_body's source over wire packets (fc_decode.hip says what a source supplies).
struct FoldWire {
  typedef WMeta Meta;
  const WireFoldArgs& a;
  const uint32_t c, base;                       // n < 2^32
  const int q;
  const uint64_t off_start, off_idx;            // val's offset depends on the packet's E
  uint32_t f0, n0, f1, n1;                      // packets lane, lane + 64: the clamped quarter
  __device__ __forceinline__ explicit FoldWire(const WireFoldArgs& a_)
      : a(a_), c(blockIdx.x), base(c * (uint32_t)kChunk), q(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)),
        off_start(kWireHdrBytes + wire_pad16(8ull * a_.nch)), off_idx(off_start + wire_pad16(4ull * a_.nch)),
        f0(0), n0(0), f1(0), n1(0) {}
  __device__ __forceinline__ const fc_packet_hdr* fill(int tid, WMeta& d) const {
    const fc_wire_job job = a.jobs[tid];
    const unsigned char* wire = static_cast<const unsigned char*>(job.wire);
    // a buffer wire_accept refuses: what the unpack makes of it, an empty packet selecting nothing
    d.wire = nullptr; d.E = 0; d.w = a.weights[tid]; d.flags = 0; d.pad_ = 0;
    if (wire == nullptr || job.bytes < kWireHdrBytes) return nullptr;
    const fc_wire_hdr* h = reinterpret_cast<const fc_wire_hdr*>(wire);
    const uint64_t E = h->n_entries;
    if (!wire_accept(h, a.n, a.nch, job.bytes, E, [](uint32_t x) { return x; })) return nullptr;
    d.wire = wire; d.E = (uint32_t)E;
    return &h->pkt;
  }
  __device__ __forceinline__ void load(const WMeta* s_meta, uint32_t M, int lane) {
    auto qload = [&](uint32_t m, uint32_t& first, uint32_t& count) {
      if (m >= M || s_meta[m].wire == nullptr) return;
      const unsigned char* wire = s_meta[m].wire;
      const WireChunk<uint32_t> k = wire_clamp(((wu64*)(wire + kWireHdrBytes))[c], ((gu32*)(wire + off_start))[c],
                                               s_meta[m].E);
      const uint32_t lo = q == 0 ? 0u : q == 1 ? k.q1 : q == 2 ? k.q2 : k.q3;
      const uint32_t hi = q == 0 ? k.q1 : q == 1 ? k.q2 : q == 2 ? k.q3 : k.cnt;
      first = k.st + lo; count = hi - lo;       // first + count <= st + cnt <= E
    };
    qload((uint32_t)lane, f0, n0);
    qload((uint32_t)lane + 64u, f1, n1);
  }
  __device__ __forceinline__ uint32_t lane_count(bool hi) const { return hi ? n1 : n0; }
  // [first, first + n) of the packet's sections.  An item with no entries (its `first` may be E,
  // its packet none) is [0, 0) of the weights: the fast body's loads read no byte of the buffer
  __device__ __forceinline__ FoldSpan span(const WMeta& pm, uint32_t m) const {   // uniform
    const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)(m < 64 ? f0 : f1), (int)(m & 63));
    const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)(m < 64 ? n0 : n1), (int)(m & 63));
    if (n == 0) return {(gu16*)a.weights, (gf32*)a.weights, 0u, 0u};
    const unsigned char* sec = uni_ptr(pm.wire) + off_idx;
    return {(gu16*)sec, (gf32*)(sec + wire_pad16(2ull * uni32(pm.E))), first, first + n};
  }
  __device__ __forceinline__ void rules(const WMeta& pm, PktCache& pk) const {
    pk.seed = 0; pk.offset = 0; pk.p = 0.0;     // no packet: nothing is read, nothing of it is used
    const fc_wire_hdr* h = (const fc_wire_hdr*)uni_ptr(pm.wire);
    if (h != nullptr) { pk.seed = h->pkt.seed; pk.offset = h->pkt.offset; pk.p = h->pkt.p; }
  }
};

template <bool ACC_IN>
__global__ __launch_bounds__(kQBlock, 4) void k_fold_wire(WireFoldArgs a) {
  FoldWire src(a);
  fold_body<ACC_IN, false>(src, a.m, a.out, a.n);
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
