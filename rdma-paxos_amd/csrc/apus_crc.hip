// CRC-32C entry digest for gfx950 (MI355X): apus_crc32c_batch and
// APUS_COMMIT_CRC32C.
//
// digest[g] = CRC-32C (Castagnoli, reflected 0x82F63B78, init and final XOR
// 0xFFFFFFFF: RFC 3720 B.4) of the byte string the Adler-32 digest covers
// (lane_group, apus_commit.hip): the concatenated spans of the entries the
// walk chain visits from commit to end, bytes 27..47 of each read as zero.
// The kernels only read the batch; they count no statistic.
//
//   crc_lane_kernel — the exact form, one LANE per group: lane_group's chain
//       loop, bytes straight from global memory (dwords where the address
//       allows), slicing-by-4 tables in LDS.  Takes any batch; also run over
//       the list of groups the wave form deferred.
//   crc_wave_kernel — the fast form, one WAVE per group, for 16-B aligned
//       rings.  The chain is cut into windows that start at an entry: the
//       window's ring bytes are staged into the wave's LDS with coalesced
//       16-B loads, the entries that lie wholly in it are found with the
//       speculative walk (lane j reads the header at m + j*elen; the chain is
//       confirmed up to the first lane that disagrees), each confirmed
//       entry's lane zeroes bytes 27..47 of the LDS copy, and the window's
//       bytes [a, m) are summed:
//         raw(M) = the CRC register run from state 0, no final XOR;
//         raw(0..0 | M) = raw(M), so the bytes are right-aligned onto 64
//         chunks of 4q bytes, lane l takes chunk l (slicing-by-4 over dword
//         LDS reads, bytes below a read as zero);
//         raw(A | B) = raw(A) * x^(8|B|) + raw(B) in GF(2)[x] mod P, so lane
//         l multiplies its chunk's register by x^(32 q (63 - l)) (one
//         32-step shift-and-XOR multiply; the multiplier from a table built
//         at compile time) and the wave XORs the 64 products;
//         a register S carried into a message is S XORed into the message's
//         first four bytes, so the running register (0xFFFFFFFF at the
//         start) enters the first two dwords of the next window and no
//         length-dependent multiply is needed between windows or at the end.
//       A wrap (header wrap or ghost header) ends a window; the next starts
//       at ring offset 0.  What the window schedule cannot settle is
//       deferred to the exact form, with the same result: rings of 2 GiB and
//       more or without 16 B of slack after len, an entry longer than a
//       window, a chain that crosses `end` or runs into the step guard.  The
//       deferred list holds n_groups entries: it cannot overflow.
#include "apus_device.h"
#include "apus_internal.h"

namespace apus {

namespace {

constexpr uint32_t kCrcPoly = 0x82F63B78u;
constexpr int kCrcWaves = 4;               // waves per 256-thread block
constexpr int kCW = 9216;                  // window bytes: 64 x 128-B entries + alignment + slack
constexpr int kCNP = kCW / 16;             // 16-B pieces per window
constexpr int kCPPL = kCNP / 64;           // pieces per lane
constexpr int kCSlots = kCNP + kCNP / 8;   // 16 B of padding after every 128 B
constexpr int kQMax = kCW / 256;           // dwords per lane of a full window
static_assert(kCNP % 64 == 0, "whole pieces per lane");

// a * b in GF(2)[x] mod P, bit-reflected operands (bit 31 is x^0)
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if ((a >> (31 - i)) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

// slicing-by-4 tables: t[k][i] = the register after byte i and k zero bytes
struct CrcTables {
    uint32_t t[4][256];
};
constexpr CrcTables make_tables()
{
    CrcTables r{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
        r.t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
        for (int k = 1; k < 4; ++k) r.t[k][i] = (r.t[k - 1][i] >> 8) ^ r.t[0][r.t[k - 1][i] & 0xFFu];
    return r;
}
// p[q][j] = x^(32 q j) mod P: lane 63 - j's multiplier when a chunk is q dwords
struct CrcPow {
    uint32_t p[kQMax + 1][64];
};
constexpr CrcPow make_pow()
{
    CrcPow r{};
    uint32_t x32 = 0x80000000u;
    for (int i = 0; i < 32; ++i) x32 = (x32 >> 1) ^ ((x32 & 1u) ? kCrcPoly : 0u);
    uint32_t xq = 0x80000000u;             // x^(32 q)
    for (int q = 0; q <= kQMax; ++q) {
        r.p[q][0] = 0x80000000u;
        for (int j = 1; j < 64; ++j) r.p[q][j] = gf_mul(r.p[q][j - 1], xq);
        xq = gf_mul(xq, x32);
    }
    return r;
}
__device__ const CrcTables d_crc_tables = make_tables();
__device__ const CrcPow d_crc_pow = make_pow();

// the tables, copied into the block's LDS (t[k] at tab + 256 k)
__device__ __forceinline__ void load_tables(uint32_t *tab)
{
    for (uint32_t i = threadIdx.x; i < 1024u; i += blockDim.x) tab[i] = d_crc_tables.t[i >> 8][i & 0xFFu];
    __syncthreads();
}
__device__ __forceinline__ uint32_t crc_byte(const uint32_t *tab, uint32_t c, uint32_t byte)
{
    return tab[(c ^ byte) & 0xFFu] ^ (c >> 8);
}
__device__ __forceinline__ uint32_t crc_word(const uint32_t *tab, uint32_t c, uint32_t w)
{
    c ^= w;
    return tab[768 + (c & 0xFFu)] ^ tab[512 + ((c >> 8) & 0xFFu)] ^ tab[256 + ((c >> 16) & 0xFFu)] ^ tab[c >> 24];
}

// ---------------------------------------------------------------------------
// the exact form
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t crc_span(const uint32_t *tab, const uint8_t *p, uint32_t n, uint32_t c)
{
    while (n && ((uintptr_t)p & 3u)) {
        c = crc_byte(tab, c, *p);
        ++p;
        --n;
    }
    for (; n >= 4; p += 4, n -= 4) c = crc_word(tab, c, *reinterpret_cast<const uint32_t *>(p));
    for (; n; ++p, --n) c = crc_byte(tab, c, *p);
    return c;
}

// lane_group's chain (apus_commit.hip), one group on one lane
__device__ __forceinline__ uint32_t crc_group(const apus_batch_t &b, uint64_t g, const uint32_t *tab)
{
    const apus_group_state_t st = load_state(b, g);
    const uint64_t len = st.len, end = st.end;
    // commit or end beyond len, len beyond the group's ring: nothing is covered.
    // A ring shorter than a header holds no entry.
    if (st.commit > len || end > len || len > ring_cap(b) || len < kHdr) return 0u;
    const uint8_t *ring = b.ring + g * b.ring_stride;
    const uint64_t guard = len / kHdr + 4;
    uint64_t m = st.commit, steps = 0;
    uint32_t c = 0xFFFFFFFFu;
    while (dist(end, len, m)) {
        if (++steps > guard) break;
        if (len - m < kHdr) m = 0;                        // log_get_entry
        const uint8_t *e = ring + m;
        const uint32_t elen = entry_len(e[kType], ld_u16(e + kData));
        if (len - m < elen) { m = 0; continue; }          // ghost header
        c = crc_span(tab, e, kSender, c);
        for (uint32_t i = kSender; i < kData; ++i) c = crc_byte(tab, c, 0u);
        c = crc_span(tab, e + kData, elen - kData, c);
        m += elen;
    }
    return ~c;
}

// every group of the batch (list == NULL) or the list[0] groups list[1..]
__global__ void __launch_bounds__(256) crc_lane_kernel(const apus_batch_t b, uint32_t *digest, const uint32_t *list)
{
    __shared__ uint32_t s_tab[1024];
    load_tables(s_tab);
    const uint64_t n = list ? (uint64_t)list[0] : b.n_groups;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t g = list ? (uint64_t)list[1 + i] : i;
        digest[g] = crc_group(b, g, s_tab);
    }
}

// ---------------------------------------------------------------------------
// the fast form
// ---------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// window byte v lives at LDS byte v + 16 (v / 128): lanes that read dwords or
// headers at a 128-B stride then hit different banks
__device__ __forceinline__ uint32_t pad_of(uint32_t v) { return v + ((v >> 7) << 4); }

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t hdr_elen(const uint8_t *win8, uint32_t rel)
{
    const uint32_t type = win8[pad_of(rel + kType)];
    const uint32_t clen = (uint32_t)win8[pad_of(rel + kData)] | ((uint32_t)win8[pad_of(rel + kData + 1)] << 8);
    return entry_len(type, clen);
}

// The register after window bytes [ra, re) (re - ra >= 8), entered with
// register s.  Uniform result.
__device__ __forceinline__ uint32_t window_crc(const uint32_t *tab, const uint8_t *win8, uint32_t lane, uint32_t ra,
                                               uint32_t re, uint32_t s)
{
    const uint32_t *win32 = reinterpret_cast<const uint32_t *>(win8);
    const int e4 = (int)(re & ~3u), a4 = (int)(ra & ~3u);
    const uint32_t sh = 8u * (ra & 3u);
    const uint32_t q = (uint32_t)((e4 - a4) / 4 + 63) / 64u;          // 1 .. kQMax
    int p = e4 - (int)((64u - lane) * 4u * q);
    uint32_t v = 0;
    for (uint32_t i = 0; i < q; ++i, p += 4) {
        uint32_t w = 0;
        if (p >= a4) {                                               // else the whole dword lies below ra
            w = win32[pad_of((uint32_t)p) >> 2];
            if (p == a4) w = (w & ~((1u << sh) - 1u)) ^ (s << sh);
            if (sh && p == a4 + 4) w ^= s >> (32u - sh);
        }
        v = crc_word(tab, v, w);
    }
    v = gf_mul(v, d_crc_pow.p[q][63u - lane]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
    v = uni(v);
    for (uint32_t t = (uint32_t)e4; t < re; ++t) v = crc_byte(tab, v, win8[pad_of(t)]);
    return uni(v);
}

__global__ void __launch_bounds__(256) crc_wave_kernel(const apus_batch_t b, uint32_t *digest, uint32_t *slow)
{
    __shared__ uint32_t s_tab[1024];
    __shared__ __attribute__((aligned(16))) uint4 s_win[kCrcWaves][kCSlots];
    load_tables(s_tab);

    const uint32_t lane = lane_id();
    const uint32_t wv = uni(threadIdx.x >> 6);
    uint4 *win = s_win[wv];
    uint8_t *win8 = reinterpret_cast<uint8_t *>(win);
    uint32_t *win32 = reinterpret_cast<uint32_t *>(win);
    const uint64_t G = b.n_groups;
    const uint64_t nw = (uint64_t)gridDim.x * kCrcWaves;
    const uint64_t cap = ring_cap(b);                    // <= ring_stride < 2^32 (launch_crc32c)

    for (uint64_t g = (uint64_t)blockIdx.x * kCrcWaves + wv; g < G; g += nw) {
        const apus_group_state_t st = load_state(b, g);
        const uint64_t len64 = uni64(st.len), end64 = uni64(st.end), commit64 = uni64(st.commit);
        uint32_t s = 0xFFFFFFFFu;
        bool defer = false;
        if (commit64 > len64 || end64 > len64 || len64 > cap || len64 < kHdr) {
            // covers nothing
        } else if (len64 >= (1ull << 31) - 16u || ((len64 + 15u) & ~15ull) > cap) {
            defer = true;
        } else {
            const uint32_t len = (uint32_t)len64, end = (uint32_t)end64;
            const uint8_t *ring = b.ring + g * b.ring_stride;
            const uint32_t guard = len / kHdr + 4;
            uint32_t m = (uint32_t)commit64, steps = 0;
            while (!defer && dist32(end, len, m) != 0) {
                if (len - m < kHdr) m = 0;                            // log_get_entry
                // the window: ring bytes [base, wlim); in a well-formed ring the
                // chain from m stays below end (or len, when it wraps first)
                const uint32_t base = m & ~15u;
                const uint32_t wlim = min(base + (uint32_t)kCW, end > m ? end : len);
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<uint8_t *>(ring), (short)0, (int)((wlim + 15u) & ~15u), 0x00020000);
                // rows of 64 pieces up to wlim (a short window stages only its
                // rows: nothing past wlim is read from LDS); pieces past wlim in
                // the last row read zero (the descriptor's range check)
                const uint32_t nrow = (wlim - base + 1023u) >> 10;
                u32x4 r[kCPPL] = {};
#pragma unroll
                for (int j = 0; j < kCPPL; ++j)
                    if ((uint32_t)j < nrow)
                        r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 16u * lane + 1024u * j, 0, 2);
                wave_sync();                         // the window before this one has been read
#pragma unroll
                for (int j = 0; j < kCPPL; ++j) {
                    const uint32_t k = lane + 64u * j;
                    if ((uint32_t)j < nrow) win[k + (k >> 3)] = make_uint4(r[j].x, r[j].y, r[j].z, r[j].w);
                }
                wave_sync();

                const uint32_t a = m;
                bool first = true, ghost = false;
                for (;;) {
                    if (!first && (dist32(end, len, m) == 0 || len - m < kHdr)) break;
                    if (m + kHdr > wlim) { defer = first; break; }
                    const uint32_t el = uni(hdr_elen(win8, m - base));
                    if (len - m < el) { ghost = true; break; }        // ghost header
                    if (m + el > wlim) { defer = first; break; }      // the next window starts here
                    // lane j: the entry at m + j * el, if the chain goes on at this length
                    const uint32_t o = m + lane * el;
                    bool ok = o + kHdr <= wlim;
                    const uint32_t elj = ok ? hdr_elen(win8, o - base) : 0u;
                    ok = ok && elj == el && o + el <= wlim && (lane == 0 || o != end);
                    const uint64_t bad = __builtin_amdgcn_ballot_w64(!ok);
                    const uint32_t k = bad ? (uint32_t)__builtin_ctzll(bad) : 64u;    // >= 1: lane 0 was checked above
                    if (lane < k) {                                   // bytes 27..47 read as zero
                        const uint32_t ro = o - base;
                        if ((ro & 3u) == 0) {
                            win8[pad_of(ro + kSender)] = 0;
#pragma unroll
                            for (uint32_t t = kReply; t < kData; t += 4) win32[pad_of(ro + t) >> 2] = 0u;
                        } else {
                            for (uint32_t t = kSender; t < kData; ++t) win8[pad_of(ro + t)] = 0;
                        }
                    }
                    steps += k;
                    m += k * el;
                    first = false;
                    if (steps > guard) { defer = true; break; }
                }
                if (defer) break;
                if (m > a) {
                    wave_sync();
                    s = window_crc(s_tab, win8, lane, a - base, m - base, s);
                }
                if (ghost) {
                    m = 0;
                    if (++steps > guard) defer = true;
                }
            }
        }
        if (lane == 0) {
            if (defer) slow[1u + atomicAdd(slow, 1u)] = (uint32_t)g;
            else digest[g] = ~s;
        }
    }
}

// the lane-per-group form for the batches the commit walk also takes on lanes
bool crc_on_lanes(const apus_batch_t &b)
{
    const bool wave_ok = ((((uintptr_t)b.ring) | b.ring_stride) & 15u) == 0 && b.ring_stride < (1ull << 32);
    return (b.flags & APUS_BATCH_LANE_IMPL) || !wave_ok;
}

}  // namespace

hipError_t launch_crc32c(apus_ctx *ctx, const apus_batch_t &b, uint32_t *digest, hipStream_t s)
{
    if (b.n_groups == 0) return hipSuccess;
    const uint32_t lgrid = grid_for(b.n_groups, 256, ctx->n_cu, 8);
    if (crc_on_lanes(b)) {
        hipLaunchKernelGGL(crc_lane_kernel, dim3(lgrid), dim3(256), 0, s, b, digest, (const uint32_t *)nullptr);
        return hipGetLastError();
    }
    ScratchPin pin;
    hipError_t e = stream_scratch(ctx, s, 1, b.n_groups, pin);
    if (e != hipSuccess) return e;
    uint32_t *slow = pin.sc->slow;                 // count (0 between launches), then the deferred groups
    const uint32_t grid = grid_for(b.n_groups, kCrcWaves, ctx->n_cu,
                                   (uint32_t)resident_blocks(ctx, 62, (const void *)crc_wave_kernel));
    hipLaunchKernelGGL(crc_wave_kernel, dim3(grid), dim3(256), 0, s, b, digest, slow);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crc_lane_kernel, dim3(lgrid), dim3(256), 0, s, b, digest, (const uint32_t *)slow);
    e = hipGetLastError();
    const hipError_t e2 = hipMemsetAsync(slow, 0, sizeof(uint32_t), s);
    return e != hipSuccess ? e : e2;
}

}  // namespace apus
