// The failure detector for gfx950 (BASELINE config 5's leader failover):
// check_failure_count (src/dare/dare_server.c:1189-1227), the heartbeat
// timer's callbacks hb_receive_cb (:822-922), hb_send_cb (:928-993) and
// to_adjust_cb (:764-817), and start_election (:1264-1322)
// (apus_gpu.h apus_failure_check_batch / apus_hb_batch /
// apus_start_election_batch).
//
// hb_kernel<false> is the exact form: one lane per group, the reference's
// loop, one atomic fetch-and per visited slot in index order.
// hb_kernel<true> is the default form.  Which slots a receive scan (or an
// adjust tick) visits is known before any heartbeat is read -- it depends on
// cid, self, sid, latest_hb and the mode -- so a block of four waves, 64
// groups per wave,
//   1. loads each lane's row inputs and leaves the lane's visit mask in LDS;
//   2. passes over the wave's 64 * R contiguous heartbeat slots, consecutive
//      lanes on consecutive slots (full lines instead of the 8R-byte lane
//      stride), fetching and clearing the visited slots only, the values
//      parked in the wave's LDS slab;
//   3. runs each lane's sequential scan over its own row from LDS;
//   4. writes the vote_ack / lr_step / send_flag rows of the groups that
//      started an election in the same slot order.
// Send-mode groups always take the exact loop (their scan stops on data:
// the slots after a step-down must stay untouched).
#include "apus_device.h"
#include "apus_group_ops.h"
#include "apus_internal.h"

namespace apus {

constexpr uint32_t kHbBlock = 256, kHbWaves = kHbBlock / 64;
constexpr uint32_t kModeElect = 0x80;     // internal: start_election alone (apus_start_election_batch)

// __sync_fetch_and_and(&hb[i], 0): read and clear in one atomic.  System
// scope: the slot's other writer is a NIC; relaxed: the slot is the only
// datum handed over.
__device__ __forceinline__ uint64_t hb_take(uint64_t *p)
{
    return __hip_atomic_fetch_and(p, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// server_update_sid (dare_server.c:2288-2297)
__device__ __forceinline__ bool sid_cas(uint64_t *p, uint64_t old_sid, uint64_t new_sid)
{
    return __hip_atomic_compare_exchange_strong(p, &old_sid, new_sid, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_SYSTEM);
}

// IS_LEADER (dare_server.c:42-48): not IS_NONE (which needs the L bit
// clear), SID_GET_IDX == idx, the L bit set
__device__ __forceinline__ bool is_leader(uint64_t sid, uint32_t self)
{
    return (uint32_t)(sid & 0xFFu) == self && APUS_SID_L(sid);
}

// start_election's SID step (dare_server.c:1270-1279): [term + 1 | 0 | self]
__device__ __forceinline__ bool election_sid(const apus_batch_t &b, uint64_t g, uint64_t sid, uint32_t self)
{
    const uint64_t ns = ((APUS_SID_TERM(sid) + 1) << 9) | (uint64_t)(self & 0xFFu);
    return sid_cas(b.sid + g, sid, ns);
}

// start_election's candidate rows (:1299-1307), slot i of group g
__device__ __forceinline__ void election_slot(const apus_batch_t &b, uint8_t *send_flag, uint64_t slot, uint64_t len)
{
    b.vote_ack[slot] = len;
    b.lr_step[slot] = APUS_LR_GET_WRITE;
    if (send_flag) send_flag[slot] = 1;
}

struct HbOut {
    uint32_t outcome, reply, n_out, from;
    bool elect;          // the SID step of start_election succeeded: the rows follow
};

// One group's tick.  fetch(i) yields the value fetched from (and cleared in)
// slot i: the atomic itself (exact form) or the staged value (default form,
// receive and adjust only).  Returns the outputs; the election rows are the
// caller's (HbOut::elect).
template <typename F>
__device__ __forceinline__ HbOut hb_group(const apus_batch_t &b, const apus_hb_io_t &io, uint64_t g, uint32_t mode,
                                          const apus_group_state_t &st, uint32_t self, uint64_t sid, uint64_t lat,
                                          uint64_t &corrupt, F fetch)
{
    const uint32_t R = b.n_replicas;
    const uint32_t size = group_size(st.cid), n = size < R ? size : R;
    HbOut o{ APUS_HB_IDLE, 0, 0, 0xFF, false };
    if (mode == kModeElect) {
        o.elect = election_sid(b, g, sid, self);
        o.outcome = o.elect ? APUS_HB_ELECTION : APUS_HB_CAS_FAILED;
    } else if (mode == APUS_HB_MODE_RECEIVE) {
        if (self >= size) {                                   // :834-839
            o.outcome = APUS_HB_NOT_MEMBER;
            return o;
        }
        offsets_of(b, g)[kOffTail] = st.len;                  // :842
        const uint32_t leader = (uint32_t)(sid & 0xFFu);
        uint64_t new_sid = sid;
        bool timeout = true;
        for (uint32_t i = 0; i < n; ++i) {
            if (i == self || !((st.cid.bitmask >> i) & 1u)) continue;
            uint64_t hb;
            if (i == leader) {                                // :849-856
                if (!lat) lat = fetch(i);
                hb = lat;
                io.latest_hb[g] = 0;
            } else {
                hb = fetch(i);                                // :859
            }
            if (hb == 0) continue;
            if (hb < new_sid) {                               // :865-879
                if (APUS_SID_L(hb)) {
                    o.reply |= 1u << i;
                    ++o.n_out;
                }
                continue;
            }
            timeout = false;                                  // :881-887
            if (APUS_SID_L(hb)) new_sid = hb;
        }
        if (timeout) {                                        // :891-896
            o.elect = election_sid(b, g, sid, self);
            o.outcome = o.elect ? APUS_HB_ELECTION : APUS_HB_CAS_FAILED;
        } else if (new_sid != sid) {                          // :898-914
            if (!sid_cas(b.sid + g, sid, new_sid)) o.outcome = APUS_HB_CAS_FAILED;
            else o.outcome = APUS_SID_TERM(sid) != APUS_SID_TERM(new_sid) ? APUS_HB_FOLLOW : APUS_HB_SID_UPDATED;
        } else {
            o.outcome = APUS_HB_REARM;
        }
    } else if (mode == APUS_HB_MODE_SEND) {
        // always the atomics in index order: the scan stops on data (:942-960)
        uint64_t *hbp = b.hb + g * R;
        o.outcome = APUS_HB_SEND;
        for (uint32_t i = 0; i < n; ++i) {
            if (i == self || !((st.cid.bitmask >> i) & 1u)) continue;
            if (hb_take(hbp + i) < sid) continue;
            o.outcome = APUS_HB_STEP_DOWN;
            o.from = i;
            break;
        }
    } else if (mode == APUS_HB_MODE_ADJUST) {
        const uint32_t leader = (uint32_t)(sid & 0xFFu);
        const uint64_t hb = leader < R ? fetch(leader) : 0ull;   // :782
        if (hb != 0) {                                        // :783-794
            io.latest_hb[g] = hb;
            if (io.leader_failed[g]) {
                io.leader_failed[g] = 0;
                o.outcome = APUS_HB_FALSE_POSITIVE;
            } else {
                o.outcome = APUS_HB_RECEIVED;
            }
        } else {                                              // :795-798
            io.leader_failed[g] = 1;
            o.outcome = APUS_HB_MISSED;
        }
    }
    if (o.outcome == APUS_HB_CAS_FAILED) ++corrupt;
    return o;
}

// the callback armed for group g: io.mode, else send for IS_LEADER groups and
// receive for the others; `due` (apus_start_election_batch) replaces both
__device__ __forceinline__ uint32_t hb_mode(const apus_hb_io_t &io, const uint8_t *due, uint64_t g, uint64_t sid,
                                            uint32_t self)
{
    if (due) return due[g] ? kModeElect : APUS_HB_MODE_IDLE;
    if (io.mode) {
        const uint32_t m = io.mode[g];
        return m <= APUS_HB_MODE_ADJUST ? m : APUS_HB_MODE_IDLE;
    }
    return is_leader(sid, self) ? APUS_HB_MODE_SEND : APUS_HB_MODE_RECEIVE;
}

// the slots of group g's row the staged pass fetches: the receive scan's
// visits (dare_server.c:846-860: i < size, not self, not OFF, the leader's
// only when latest_hb is 0), the adjust tick's leader slot (:782)
__device__ __forceinline__ uint32_t visit_mask(uint32_t mode, const apus_group_state_t &st, uint32_t R, uint32_t self,
                                               uint64_t sid, uint64_t lat)
{
    const uint32_t leader = (uint32_t)(sid & 0xFFu);
    if (mode == APUS_HB_MODE_ADJUST) return leader < R ? 1u << leader : 0u;
    if (mode != APUS_HB_MODE_RECEIVE) return 0u;
    const uint32_t size = group_size(st.cid), n = size < R ? size : R;
    if (self >= size) return 0u;
    uint32_t m = st.cid.bitmask & ((1u << n) - 1u);
    if (self < 32u) m &= ~(1u << self);
    if (lat != 0 && leader < 32u) m &= ~(1u << leader);
    return m;
}

__device__ __forceinline__ void hb_store(const apus_hb_io_t &io, uint64_t g, const HbOut &o)
{
    io.outcome[g] = (uint8_t)o.outcome;
    if (io.reply) io.reply[g] = (uint16_t)o.reply;
    if (io.n_outdated) io.n_outdated[g] = (uint8_t)o.n_out;
    if (io.from) io.from[g] = (uint8_t)o.from;
}

template <bool COOP>
__global__ void __launch_bounds__(kHbBlock) hb_kernel(const apus_batch_t b, const apus_hb_io_t io, const uint8_t *due,
                                                      uint64_t *stats)
{
    // per wave: 64 * R staged heartbeats, then 64 election lengths (0: none),
    // then 64 visit masks / election sizes
    extern __shared__ uint64_t lds[];
    const uint32_t R = b.n_replicas;
    const uint64_t G = b.n_groups;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t *const slab = lds + (uint64_t)wave * (64u * R + 64u + 32u);
    uint64_t *const elen = slab + 64u * R;
    uint32_t *const mask = reinterpret_cast<uint32_t *>(elen + 64);
    uint64_t corrupt = 0;
    // every thread of the block runs every round (the barriers below)
    for (uint64_t base = (uint64_t)blockIdx.x * kHbBlock; base < G; base += (uint64_t)gridDim.x * kHbBlock) {
        const uint64_t gb = base + (uint64_t)wave * 64u;          // the wave's first group
        const uint32_t ng = gb < G ? (uint32_t)(G - gb < 64u ? G - gb : 64u) : 0u;
        const uint64_t g = gb + lane;
        const bool live = lane < ng;
        apus_group_state_t st{};
        uint32_t self = 0, mode = APUS_HB_MODE_IDLE;
        uint64_t sid = 0, lat = 0;
        if (live) {
            st = load_state(b, g);
            self = b.self_idx[g];
            sid = b.sid[g];
            mode = hb_mode(io, due, g, sid, self);
            if (mode == APUS_HB_MODE_RECEIVE) lat = io.latest_hb[g];
        }
        HbOut o{};
        if (COOP) {
            mask[lane] = live ? visit_mask(mode, st, R, self, sid, lat) : 0u;
            __syncthreads();
            // 2. the wave's rows, slot by slot: k = (group - gb) * R + i < ng * R
            uint64_t *const row = b.hb + gb * R;
            for (uint32_t k = lane; k < ng * R; k += 64u) {
                const uint32_t gl = k / R, i = k - gl * R;
                if ((mask[gl] >> i) & 1u) slab[k] = hb_take(row + k);
            }
            __syncthreads();
            // 3. the scans, from LDS
            if (live) {
                const uint64_t *mine = slab + lane * R;
                o = hb_group(b, io, g, mode, st, self, sid, lat, corrupt, [&](uint32_t i) { return mine[i]; });
                hb_store(io, g, o);
            }
            // 4. the election rows
            const uint32_t size = group_size(st.cid);
            mask[lane] = live && o.elect ? (size < R ? size : R) : 0u;
            elen[lane] = st.len;
            const bool any = __ballot(live && o.elect) != 0;      // wave-uniform
            __syncthreads();
            if (any) {
                for (uint32_t k = lane; k < ng * R; k += 64u) {
                    const uint32_t gl = k / R, i = k - gl * R;
                    if (i < mask[gl]) election_slot(b, io.send_flag, gb * R + k, elen[gl]);
                }
            }
            __syncthreads();                                      // mask / slab are rewritten next round
        } else if (live) {
            uint64_t *hbp = b.hb + g * R;
            o = hb_group(b, io, g, mode, st, self, sid, lat, corrupt, [&](uint32_t i) { return hb_take(hbp + i); });
            hb_store(io, g, o);
            if (o.elect) {
                const uint32_t size = group_size(st.cid), n = size < R ? size : R;
                for (uint32_t i = 0; i < n; ++i) election_slot(b, io.send_flag, g * R + i, st.len);
            }
        }
    }
    if (corrupt) atomicAdd((unsigned long long *)&stats[APUS_STAT_CORRUPT], (unsigned long long)corrupt);
}

// check_failure_count (dare_server.c:1189-1227), one lane per group; the rare
// appending lanes call append_bare, as vote_win_kernel does
__global__ void __launch_bounds__(256) failure_check_kernel(const apus_batch_t b, const apus_fail_io_t io,
                                                            uint64_t *stats)
{
    const uint32_t R = b.n_replicas;
    uint64_t corrupt = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < b.n_groups;
         g += (uint64_t)gridDim.x * blockDim.x) {
        apus_group_state_t st = load_state(b, g);
        const uint32_t self = b.self_idx[g];
        const uint64_t sid = b.sid[g];
        const uint8_t *fail = b.fail_count + g * R;
        const uint32_t size = group_size(st.cid), n = size < R ? size : R;
        const bool leader = is_leader(sid, self);
        const bool can_remove = leader && st.cid.state == APUS_CID_STABLE;      // :1202
        uint32_t copy = st.cid.bitmask, conn = 0, removed = 0;
        for (uint32_t i = 0; i < n; ++i) {                                      // :1196-1212
            if (!((copy >> i) & 1u)) continue;
            if (fail[i] >= APUS_PERMANENT_FAILURE) {
                if (can_remove) {
                    copy &= ~(1u << i);                                         // CID_SERVER_RM
                    removed |= 1u << i;
                }
            } else {
                ++conn;
            }
        }
        uint32_t action = APUS_FAIL_NONE;
        uint64_t cfg = 0;
        if ((conn & 0xFFu) <= size / 2) {                                       // :1213-1217
            action = APUS_FAIL_SHUTDOWN;
        } else if (leader && copy != st.cid.bitmask) {                          // :1218-1226
            if (!append_ok(b, st)) {
                action = APUS_FAIL_REFUSED;
                ++corrupt;
            } else {
                action = APUS_FAIL_REMOVED;
                st.cid.bitmask = copy;
                uint64_t w[2];
                __builtin_memcpy(w, &st.cid, sizeof w);
                cid_words(b, g)[1] = w[1];
                io.req_id[g] = 0;
                io.clt_id[g] = 0;
                uint32_t prev = b.prev_head ? b.prev_head[g] : 0u;
                bool stopped = false;
                cfg = append_bare(b, g, st, prev, APUS_SID_TERM(sid), APUS_CONFIG, 0, 0, w, stopped);
                if (b.prev_head) b.prev_head[g] = (uint8_t)prev;
            }
        }
        io.action[g] = (uint8_t)action;
        io.connections[g] = (uint8_t)conn;
        if (io.removed) io.removed[g] = (uint16_t)removed;
        if (io.cfg_idx) io.cfg_idx[g] = cfg;
    }
    if (corrupt) atomicAdd((unsigned long long *)&stats[APUS_STAT_CORRUPT], (unsigned long long)corrupt);
}

hipError_t launch_hb(apus_ctx *ctx, const apus_batch_t &b, const apus_hb_io_t &io, const uint8_t *due, hipStream_t s)
{
    if (!b.n_groups) return hipSuccess;
    if (b.n_groups >> 32) return hipErrorInvalidValue;
    const uint32_t grid = grid_for(b.n_groups, kHbBlock, ctx->n_cu, 8);
    if (b.flags & APUS_BATCH_LANE_IMPL) {
        hipLaunchKernelGGL(hb_kernel<false>, dim3(grid), dim3(kHbBlock), 0, s, b, io, due, ctx->stats);
    } else {
        const size_t lds = (size_t)kHbWaves * (64u * b.n_replicas + 64u + 32u) * sizeof(uint64_t);
        hipLaunchKernelGGL(hb_kernel<true>, dim3(grid), dim3(kHbBlock), lds, s, b, io, due, ctx->stats);
    }
    return hipGetLastError();
}

hipError_t launch_failure_check(apus_ctx *ctx, const apus_batch_t &b, const apus_fail_io_t &io, hipStream_t s)
{
    if (!b.n_groups) return hipSuccess;
    const uint32_t grid = grid_for(b.n_groups, 256, ctx->n_cu, 8);
    hipLaunchKernelGGL(failure_check_kernel, dim3(grid), dim3(256), 0, s, b, io, ctx->stats);
    return hipGetLastError();
}

}  // namespace apus
