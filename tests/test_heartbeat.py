"""The failure detector (BASELINE config 5's leader failover):
check_failure_count (src/dare/dare_server.c:1189-1227), hb_receive_cb
(:822-922), hb_send_cb (:928-993), to_adjust_cb (:764-817) and start_election
(:1264-1322) -- apus_failure_check_batch, apus_hb_batch and
apus_start_election_batch.

The reference here is a line-by-line Python restatement of those five
functions (re_* below, every branch with its reference line); the CONFIG
append of check_failure_count goes through the oracle's log_append_entry
(orc.append, one CONFIG record per REMOVED group).  It is not yet pinned by
oracle/_ref drift regions.  As the library, it never visits a
server i >= n_replicas (no column), and it gives APUS_HB_MODE_ADJUST with
SID_GET_IDX(sid) >= n_replicas the MISSED outcome without a read.

CPU: the restatement on hand-derived scenarios; the header's constants, the
exports and the NULL-argument refusals of the three entry points.
GPU: random batches in both kernel forms, on state rows and dare_log_t
images, explicit and derived modes, aligned and misaligned columns; the
failure check on generated rings; the whole election cycle; heartbeats landed
from a second stream.  Every comparison is exact.

No racing writer exists in these tests (a race is not testable bit-exactly),
so APUS_HB_CAS_FAILED is the one outcome never produced; with mode = NULL the
adjust outcomes and APUS_HB_IDLE cannot occur either.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "apus_gpu.h")

PERMANENT_FAILURE, LR_GET_WRITE, CONFIG = 2, 1, 2
STABLE, TRANSIT, EXTENDED = 0, 1, 2
(IDLE, NOT_MEMBER, REARM, ELECTION, SID_UPDATED, FOLLOW, CAS_FAILED, SEND, STEP_DOWN, RECEIVED, FALSE_POSITIVE,
 MISSED) = range(12)
M_IDLE, M_RECEIVE, M_SEND, M_ADJUST = range(4)
F_NONE, F_SHUTDOWN, F_REMOVED, F_REFUSED = range(4)


# ------------------------------------------------------------ restatement
def sid_of(term, leader, idx):
    return (term << 9) | (int(bool(leader)) << 8) | idx


def SID_L(s):                                   # dare_server.h:56
    return (s >> 8) & 1


def SID_TERM(s):                                # dare_server.h:60
    return s >> 9


def SID_IDX(s):                                 # dare_server.h:53
    return s & 0xFF


def group_size(cid):                            # dare_config.h:89-97
    s0, s1 = int(cid["size0"]), int(cid["size1"])
    if int(cid["state"]) != TRANSIT:
        return s0
    return s1 if s0 < s1 else s0


def is_on(cid, i):                              # dare_config.h:26
    return (int(cid["bitmask"]) >> i) & 1


def is_leader(sid, idx):                        # dare_server.c:42-48
    none = SID_IDX(sid) == idx and not SID_L(sid) and SID_TERM(sid) == 0
    return (not none) and SID_IDX(sid) == idx and bool(SID_L(sid))


def hb_io(G, R, mode=None, latest_hb=None, leader_failed=None, send_flag=None):
    """host arrays of apus_hb_io_t (copies; the dict is updated in place)"""
    def c(a, n, dt):
        return np.zeros(n, dt) if a is None else np.array(a, dt).copy()
    return {"mode": None if mode is None else np.array(mode, np.uint8).copy(),
            "latest_hb": c(latest_hb, G, np.uint64), "leader_failed": c(leader_failed, G, np.uint8),
            "send_flag": c(send_flag, G * R, np.uint8), "outcome": np.zeros(G, np.uint8),
            "reply": np.zeros(G, np.uint16), "n_outdated": np.zeros(G, np.uint8), "from": np.full(G, 0, np.uint8)}


def fetch_and_clear(hb, slot):                  # __sync_fetch_and_and(&hb[i], 0)
    v = int(hb.hb[slot])
    hb.hb[slot] = 0
    return v


def re_start_election(hb, io, g):
    """start_election, dare_server.c:1264-1322 (no racing writer: the
    compare-and-swap of :1276 succeeds)"""
    R = hb.R
    st = hb.state[g]
    sid = int(hb.sid[g])
    hb.sid[g] = sid_of(SID_TERM(sid) + 1, 0, int(hb.self_idx[g]))      # :1270-1276
    size = group_size(st["cid"])                                       # :1299
    for i in range(min(size, R)):                                      # :1300-1307
        hb.vote_ack[g * R + i] = st["len"]
        hb.lr_step[g * R + i] = LR_GET_WRITE
        io["send_flag"][g * R + i] = 1
    return ELECTION


def re_hb_receive(hb, io, g):
    """hb_receive_cb, dare_server.c:822-922"""
    R = hb.R
    st = hb.state[g]
    self_idx = int(hb.self_idx[g])
    size = group_size(st["cid"])                                       # :832
    if self_idx >= size:                                               # :834-839
        return NOT_MEMBER
    hb.state["tail"][g] = st["len"]                                    # :842
    sid = int(hb.sid[g])
    leader = SID_IDX(sid)                                              # :844
    new_sid = sid                                                      # :845
    timeout = True
    for i in range(min(size, R)):                                      # :846
        if i == self_idx or not is_on(st["cid"], i):                   # :847-848
            continue
        if i == leader:                                                # :849-856
            if not int(io["latest_hb"][g]):
                io["latest_hb"][g] = fetch_and_clear(hb, g * R + i)
            v = int(io["latest_hb"][g])
            io["latest_hb"][g] = 0
        else:
            v = fetch_and_clear(hb, g * R + i)                         # :859
        if v == 0:                                                     # :861-864
            continue
        if v < new_sid:                                                # :865-879
            if SID_L(v):
                io["reply"][g] |= 1 << i                               # :874
                io["n_outdated"][g] += 1                               # :876
            continue
        timeout = False                                                # :882
        if SID_L(v):                                                   # :884-887
            new_sid = v
    if timeout:                                                        # :891-896
        return re_start_election(hb, io, g)
    if new_sid != sid:                                                 # :898-914
        hb.sid[g] = new_sid
        return FOLLOW if SID_TERM(sid) != SID_TERM(new_sid) else SID_UPDATED
    return REARM                                                       # :916-921


def re_hb_send(hb, io, g):
    """hb_send_cb, dare_server.c:928-993"""
    R = hb.R
    st = hb.state[g]
    self_idx = int(hb.self_idx[g])
    new_sid = int(hb.sid[g])                                           # :935
    size = group_size(st["cid"])                                       # :940
    for i in range(min(size, R)):                                      # :942
        if i == self_idx or not is_on(st["cid"], i):                   # :943-944
            continue
        v = fetch_and_clear(hb, g * R + i)                             # :947
        if v < new_sid:                                                # :948
            continue
        io["from"][g] = i                                              # :951-959: the SID swapped for itself
        return STEP_DOWN
    return SEND                                                        # :963


def re_to_adjust(hb, io, g):
    """to_adjust_cb, dare_server.c:764-817"""
    R = hb.R
    leader = SID_IDX(int(hb.sid[g]))                                   # :770
    v = fetch_and_clear(hb, g * R + leader) if leader < R else 0       # :782 (hb[] has R columns)
    if v != 0:                                                         # :783-794
        io["latest_hb"][g] = v
        if io["leader_failed"][g]:
            io["leader_failed"][g] = 0
            return FALSE_POSITIVE
        return RECEIVED
    io["leader_failed"][g] = 1                                         # :795-798
    return MISSED


def re_hb(hb, io):
    """apus_hb_batch over a host batch, in place on hb and io"""
    for g in range(hb.G):
        io["reply"][g] = 0
        io["n_outdated"][g] = 0
        io["from"][g] = 0xFF
        if io["mode"] is not None:
            mode = int(io["mode"][g])
        else:
            mode = M_SEND if is_leader(int(hb.sid[g]), int(hb.self_idx[g])) else M_RECEIVE
        fn = {M_RECEIVE: re_hb_receive, M_SEND: re_hb_send, M_ADJUST: re_to_adjust}.get(mode)
        io["outcome"][g] = IDLE if fn is None else fn(hb, io, g)


def re_elect(hb, io):
    """apus_start_election_batch: start_election where due"""
    for g in range(hb.G):
        io["outcome"][g] = re_start_election(hb, io, g) if io["due"][g] else IDLE


def fail_io(G, req_id=None, clt_id=None):
    def c(a, n, dt):
        return np.zeros(n, dt) if a is None else np.array(a, dt).copy()
    return {"req_id": c(req_id, G, np.uint64), "clt_id": c(clt_id, G, np.uint16), "action": np.zeros(G, np.uint8),
            "connections": np.zeros(G, np.uint8), "removed": np.zeros(G, np.uint16),
            "cfg_idx": np.zeros(G, np.uint64)}


def re_check_failure_count(pkg, orc, hb, io):
    """check_failure_count, dare_server.c:1189-1227, over a host batch (in
    place); the CONFIG appends by the oracle's log_append_entry.  Returns the
    number of REFUSED groups."""
    G, R = hb.G, hb.R
    ent = np.zeros(G, pkg.batch.APPEND_DT)
    ent["type"] = CONFIG
    ent["data_off"] = np.arange(G, dtype=np.uint64) * 16
    payload = np.zeros(G * 16, np.uint8)
    n = np.zeros(G, np.uint32)
    refused = 0
    for g in range(G):
        st = hb.state[g]
        cid = st["cid"]
        sid = int(hb.sid[g])
        leader = is_leader(sid, int(hb.self_idx[g]))
        size = group_size(cid)                                         # :1193
        mask = int(cid["bitmask"])                                     # :1195
        connections = removed = 0
        for i in range(min(size, R)):                                  # :1196
            if not (mask >> i) & 1:                                    # :1197
                continue
            if hb.fail_count[g * R + i] >= PERMANENT_FAILURE:          # :1198
                if leader and int(cid["state"]) == STABLE:             # :1202
                    removed |= 1 << i                                  # :1203
                    mask &= ~(1 << i)                                  # :1204
            else:
                connections += 1                                       # :1210
        io["connections"][g] = connections
        io["removed"][g] = removed
        io["cfg_idx"][g] = 0
        if connections <= size // 2:                                   # :1213-1217
            io["action"][g] = F_SHUTDOWN
            continue
        if leader and mask != int(cid["bitmask"]):                     # :1218
            ln = int(st["len"])
            if not (64 <= ln <= hb.stride and int(st["end"]) <= ln and int(st["tail"]) <= ln):
                io["action"][g] = F_REFUSED                            # offsets the batched append refuses
                refused += 1
                continue
            hb.state["cid"]["bitmask"][g] = mask                       # :1221
            io["req_id"][g] = 0                                        # :1222
            io["clt_id"][g] = 0                                        # :1223
            payload[16 * g:16 * g + 16] = np.frombuffer(hb.state["cid"][g].tobytes(), np.uint8)
            n[g] = 1                                                   # :1224-1225
            io["action"][g] = F_REMOVED
        else:
            io["action"][g] = F_NONE
    if n.any():
        term = (hb.sid >> np.uint64(9)).astype(np.uint64)
        idx, _, bad = orc.append(hb, ent, payload, 1, n_entries=n, term=term)
        assert bad == 0
        io["cfg_idx"][:] = idx
    return refused


# ------------------------------------------------------------- scenarios
def scen(orc, R=3, state=STABLE, size=(3, 0), mask=0b111, self_idx=1, sid=2816, hb=(), ln=4096, **kw):
    """one group as the issue's table sets it up"""
    b = orc.host_batch(1, R, ln)
    st = b.state
    st["len"] = ln
    st["end"] = st["tail"] = 128
    st["cid"]["size0"], st["cid"]["size1"] = size
    st["cid"]["state"] = state
    st["cid"]["bitmask"] = mask
    st["cid"]["epoch"] = 7
    b.self_idx[:] = self_idx
    b.sid[:] = sid
    b.hb[:len(hb)] = hb
    b.vote_ack[:] = 11
    b.lr_step[:] = 5
    return b, hb_io(1, R, **kw)


def test_sid_layout():
    assert sid_of(5, 1, 0) == 2816 and sid_of(6, 0, 1) == 3073 and sid_of(4, 1, 2) == 2306
    assert sid_of(7, 1, 2) == 3842 and sid_of(6, 0, 2) == 3074 and sid_of(6, 1, 2) == 3330
    assert sid_of(5, 0, 1) == 2561 and sid_of(5, 0, 2) == 2562 and sid_of(7, 0, 1) == 3585


def test_receive_rearm(orc):
    b, io = scen(orc, hb=[2816, 0, 0], mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["outcome"][0] == REARM and not b.hb.any() and b.state["tail"][0] == 4096
    assert b.sid[0] == 2816 and io["reply"][0] == 0 and io["from"][0] == 0xFF


def test_receive_timeout_starts_election(orc):
    b, io = scen(orc, mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["outcome"][0] == ELECTION and b.sid[0] == 3073
    assert b.vote_ack.tolist() == [4096] * 3 and b.lr_step.tolist() == [1, 1, 1]
    assert io["send_flag"].tolist() == [1, 1, 1]


def test_receive_outdated_leader_then_election(orc):
    b, io = scen(orc, hb=[0, 0, 2306], mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["reply"][0] == 0b100 and io["n_outdated"][0] == 1 and io["outcome"][0] == ELECTION
    assert b.sid[0] == 3073 and not b.hb.any()


def test_receive_follow(orc):
    b, io = scen(orc, hb=[0, 0, 3842], mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["outcome"][0] == FOLLOW and b.sid[0] == 3842


def test_receive_sid_updated(orc):
    b, io = scen(orc, sid=3074, hb=[0, 0, 3330], mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["outcome"][0] == SID_UPDATED and b.sid[0] == 3330


def test_receive_latest_hb_spares_the_slot(orc):
    b, io = scen(orc, hb=[2816, 0, 0], mode=[M_RECEIVE], latest_hb=[2816])
    re_hb(b, io)
    assert io["outcome"][0] == REARM and b.hb[0] == 2816 and io["latest_hb"][0] == 0


def test_receive_up_to_date_without_leader_bit(orc):
    b, io = scen(orc, sid=2561, hb=[0, 0, 2562], mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["outcome"][0] == REARM and b.sid[0] == 2561


def test_receive_not_member(orc):
    b, io = scen(orc, state=EXTENDED, size=(2, 3), self_idx=2, hb=[2816, 5, 0], mode=[M_RECEIVE])
    b.state["tail"] = 64
    re_hb(b, io)
    assert io["outcome"][0] == NOT_MEMBER and b.state["tail"][0] == 64
    assert b.hb.tolist() == [2816, 5, 0] and b.sid[0] == 2816


def test_receive_off_server_untouched(orc):
    b, io = scen(orc, mask=0b011, hb=[0, 0, 3842], mode=[M_RECEIVE])
    re_hb(b, io)
    assert io["outcome"][0] == ELECTION and b.hb[2] == 3842


def test_send(orc):
    b, io = scen(orc, self_idx=0, hb=[0, 5, 0], mode=[M_SEND])
    re_hb(b, io)
    assert io["outcome"][0] == SEND and not b.hb.any() and b.sid[0] == 2816


def test_send_step_down_stops_the_scan(orc):
    b, io = scen(orc, self_idx=0, hb=[0, 3585, 9], mode=[M_SEND])
    re_hb(b, io)
    assert io["outcome"][0] == STEP_DOWN and io["from"][0] == 1
    assert b.hb.tolist() == [0, 0, 9] and b.sid[0] == 2816


def test_derived_mode(orc):
    """mode NULL: SEND for IS_LEADER groups, RECEIVE for the others"""
    b, io = scen(orc, self_idx=0, hb=[0, 5, 0])
    re_hb(b, io)
    assert io["outcome"][0] == SEND
    b, io = scen(orc, self_idx=1, hb=[2816, 0, 0])
    re_hb(b, io)
    assert io["outcome"][0] == REARM


def test_adjust(orc):
    b, io = scen(orc, hb=[2816, 0, 0], mode=[M_ADJUST])
    re_hb(b, io)
    assert io["outcome"][0] == RECEIVED and io["latest_hb"][0] == 2816 and b.hb[0] == 0
    b, io = scen(orc, hb=[2816, 0, 0], mode=[M_ADJUST], leader_failed=[1])
    re_hb(b, io)
    assert io["outcome"][0] == FALSE_POSITIVE and io["leader_failed"][0] == 0 and io["latest_hb"][0] == 2816
    b, io = scen(orc, hb=[0, 7, 7], mode=[M_ADJUST])
    re_hb(b, io)
    assert io["outcome"][0] == MISSED and io["leader_failed"][0] == 1 and b.hb.tolist() == [0, 7, 7]


def test_start_election_alone(orc):
    b, io = scen(orc)
    io = {"due": np.array([1], np.uint8), "send_flag": np.zeros(3, np.uint8), "outcome": np.zeros(1, np.uint8)}
    re_elect(b, io)
    assert io["outcome"][0] == ELECTION and b.sid[0] == 3073 and io["send_flag"].tolist() == [1, 1, 1]


def _fail_scen(pkg, orc, self_idx, fail, state=STABLE):
    b, _ = scen(orc, R=5, size=(5, 0), mask=0b11111, self_idx=self_idx, state=state)
    b.fail_count[:] = fail
    io = fail_io(1, req_id=[77], clt_id=[9])
    return b, io, re_check_failure_count(pkg, orc, b, io)


def test_failure_check_leader_removes(pkg, orc):
    b, io, refused = _fail_scen(pkg, orc, 0, [0, 0, 2, 0, 3])
    assert io["connections"][0] == 3 and io["removed"][0] == 0b10100 and io["action"][0] == F_REMOVED
    assert b.state["cid"]["bitmask"][0] == 0b01011 and io["req_id"][0] == 0 and io["clt_id"][0] == 0
    assert refused == 0 and b.state["end"][0] == 192 and b.state["tail"][0] == 128 and io["cfg_idx"][0] != 0
    e = b.ring[128:192]
    assert e[26] == CONFIG and int.from_bytes(e[8:16].tobytes(), "little") == 5        # SID_GET_TERM(2816)
    assert e[48:64].tobytes() == b.state["cid"][0:1].tobytes()


def test_failure_check_follower(pkg, orc):
    b, io, _ = _fail_scen(pkg, orc, 1, [0, 0, 2, 0, 3])
    assert io["action"][0] == F_NONE and io["connections"][0] == 3 and io["removed"][0] == 0
    assert b.state["cid"]["bitmask"][0] == 0b11111 and io["req_id"][0] == 77 and b.state["end"][0] == 128


def test_failure_check_shutdown(pkg, orc):
    b, io, _ = _fail_scen(pkg, orc, 0, [0, 2, 2, 2, 0])
    assert io["action"][0] == F_SHUTDOWN and io["removed"][0] == 0b01110 and io["connections"][0] == 2
    assert b.state["cid"]["bitmask"][0] == 0b11111 and b.state["end"][0] == 128 and not b.ring.any()


def test_failure_check_transit_leader(pkg, orc):
    b, io, _ = _fail_scen(pkg, orc, 0, [0, 0, 2, 0, 0], state=TRANSIT)
    assert io["action"][0] == F_NONE and io["removed"][0] == 0 and io["connections"][0] == 4
    assert b.state["cid"]["bitmask"][0] == 0b11111


# ------------------------------------------------------- the C ABI, no GPU
NEW_CONSTANTS = ("FAIL_NONE", "FAIL_SHUTDOWN", "FAIL_REMOVED", "FAIL_REFUSED", "HB_MODE_IDLE", "HB_MODE_RECEIVE",
                 "HB_MODE_SEND", "HB_MODE_ADJUST", "HB_IDLE", "HB_NOT_MEMBER", "HB_REARM", "HB_ELECTION",
                 "HB_SID_UPDATED", "HB_FOLLOW", "HB_CAS_FAILED", "HB_SEND", "HB_STEP_DOWN", "HB_RECEIVED",
                 "HB_FALSE_POSITIVE", "HB_MISSED")
NEW_ENTRIES = ("apus_failure_check_batch", "apus_hb_batch", "apus_start_election_batch")


def test_header_constants_equal_ctypes_mirror(pkg):
    abi = pkg.abi
    text = open(HEADER).read()
    vals = {n: int(v, 0) for n, v in re.findall(r"^#define\s+APUS_([A-Z0-9_]+)\s+(\d+)", text, re.M)}
    for name in NEW_CONSTANTS:
        assert getattr(abi, name) == vals[name], name
    # this file's own codes are the header's
    assert [vals[n] for n in NEW_CONSTANTS[:4]] == [F_NONE, F_SHUTDOWN, F_REMOVED, F_REFUSED]
    assert [vals[n] for n in NEW_CONSTANTS[4:8]] == [M_IDLE, M_RECEIVE, M_SEND, M_ADJUST]
    assert [vals[n] for n in NEW_CONSTANTS[8:]] == list(range(12))
    assert vals["ABI_VERSION"] == 7 and vals["STAT_COUNT"] == 9
    assert C.sizeof(abi.FailIO) == 48 and C.sizeof(abi.HbIO) == 64 and C.sizeof(abi.Batch) == 168


def test_entries_exported_and_listed(pkg):
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    exported = set(re.findall(r"\bT (apus_\w+)", nm))
    listed = {n for n, _, _ in pkg.abi.SIGNATURES}
    for name in NEW_ENTRIES:
        assert name in exported and name in listed, name


def test_null_arguments_refused(pkg):
    """no context, batch, I/O struct or required column: APUS_ERROR before
    anything is touched (runs without a GPU)"""
    abi = pkg.abi
    lib = abi.load_library()
    ctx = C.c_void_p(8)                          # never dereferenced: a later check fails first
    one = np.zeros(64, np.uint64)
    p = one.ctypes.data
    assert lib.apus_failure_check_batch(None, None, None, None) == abi.APUS_ERROR
    assert lib.apus_hb_batch(None, None, None, None) == abi.APUS_ERROR
    assert lib.apus_start_election_batch(None, None, None, None, None, None) == abi.APUS_ERROR
    full = dict(n_groups=1, n_replicas=3, ring_stride=64, ring=p, state=p, self_idx=p, sid=p, hb=p, vote_ack=p,
                lr_step=p, fail_count=p)
    fio = abi.FailIO(req_id=p, clt_id=p, action=p, connections=p)
    hio = abi.HbIO(latest_hb=p, leader_failed=p, outcome=p, reply=p, n_outdated=p, from_=p)
    b = abi.Batch(**full)
    assert lib.apus_failure_check_batch(ctx, None, C.byref(fio), None) == abi.APUS_ERROR
    assert lib.apus_failure_check_batch(ctx, C.byref(b), None, None) == abi.APUS_ERROR
    assert lib.apus_failure_check_batch(None, C.byref(b), C.byref(fio), None) == abi.APUS_ERROR
    assert lib.apus_hb_batch(ctx, None, C.byref(hio), None) == abi.APUS_ERROR
    assert lib.apus_hb_batch(ctx, C.byref(b), None, None) == abi.APUS_ERROR
    assert lib.apus_hb_batch(None, C.byref(b), C.byref(hio), None) == abi.APUS_ERROR
    assert lib.apus_start_election_batch(ctx, None, p, p, p, None) == abi.APUS_ERROR
    assert lib.apus_start_election_batch(ctx, C.byref(b), None, p, p, None) == abi.APUS_ERROR
    assert lib.apus_start_election_batch(ctx, C.byref(b), p, p, None, None) == abi.APUS_ERROR
    for col in ("ring", "sid", "fail_count", "self_idx", "state"):
        assert lib.apus_failure_check_batch(ctx, C.byref(abi.Batch(**{**full, col: None})), C.byref(fio),
                                            None) == abi.APUS_ERROR, col
    for col in ("sid", "hb", "vote_ack", "lr_step", "self_idx", "state"):
        assert lib.apus_hb_batch(ctx, C.byref(abi.Batch(**{**full, col: None})), C.byref(hio),
                                 None) == abi.APUS_ERROR, col
    for col in ("sid", "vote_ack", "lr_step"):
        assert lib.apus_start_election_batch(ctx, C.byref(abi.Batch(**{**full, col: None})), p, p, p,
                                             None) == abi.APUS_ERROR, col
    for f in ("req_id", "clt_id", "action", "connections"):
        io = abi.FailIO(**{k: (None if k == f else p) for k in ("req_id", "clt_id", "action", "connections")})
        assert lib.apus_failure_check_batch(ctx, C.byref(b), C.byref(io), None) == abi.APUS_ERROR, f
    for f in ("latest_hb", "leader_failed", "outcome", "reply", "n_outdated", "from_"):
        io = abi.HbIO(**{k: (None if k == f else p)
                         for k in ("latest_hb", "leader_failed", "outcome", "reply", "n_outdated", "from_")})
        assert lib.apus_hb_batch(ctx, C.byref(b), C.byref(io), None) == abi.APUS_ERROR, f


# ------------------------------------------------------- random batches
GS, RS = (1, 63, 64, 65, 257, 1000), (3, 5, 7, 13)
RING_LEN = 256
HB_OUT = ("outcome", "reply", "n_outdated", "from", "latest_hb", "leader_failed", "send_flag")
HB_WRITTEN = ("hb", "sid", "vote_ack", "lr_step", "state")
HB_UNCHANGED = ("remote_end", "remote_commit", "apply_offsets", "fail_count")
EXPLICIT_OUTCOMES = {IDLE, NOT_MEMBER, REARM, ELECTION, SID_UPDATED, FOLLOW, SEND, STEP_DOWN, RECEIVED,
                     FALSE_POSITIVE, MISSED}
DERIVED_OUTCOMES = {NOT_MEMBER, REARM, ELECTION, SID_UPDATED, FOLLOW, SEND, STEP_DOWN}


def random_hb_case(orc, G, R, explicit, seed=0):
    """a seeded batch for apus_hb_batch: SIDs of every role, heartbeats within
    +-2 terms of the SID with and without L (zero with p ~ 0.4 over the batch:
    a group's own rate is 0.1, 0.4 or 0.95 -- a leader whose followers are
    quiet is the common SEND case), latest_hb set with p ~ 0.2, every cid
    state, OFF servers, self beyond the group size, sizes beyond R"""
    rng = np.random.default_rng(1000 * G + 10 * R + int(explicit) + 7919 * seed)
    hb = orc.host_batch(G, R, RING_LEN)
    hb.ring[:] = rng.integers(0, 256, hb.ring.size, dtype=np.uint8)
    st = hb.state
    st["len"] = RING_LEN
    st["head"] = st["apply"] = st["commit"] = 0
    st["end"] = 64 * rng.integers(0, 4, G)
    st["tail"] = np.where(rng.random(G) < 0.5, RING_LEN, 0)
    cid = st["cid"]
    cid["epoch"] = rng.integers(0, 100, G)
    cid["state"] = rng.integers(0, 3, G)
    top = min(13, R + 1)
    cid["size0"] = rng.integers(1, top + 1, G)
    cid["size1"] = np.where(cid["state"] == STABLE, 0, rng.integers(0, top + 1, G))
    cid["bitmask"] = np.bitwise_or.reduce((rng.random((G, 13)) < 0.85).astype(np.uint32) << np.arange(13, dtype=np.uint32),
                                          axis=1)
    hb.self_idx[:] = rng.integers(0, R + 1, G)
    self_idx = hb.self_idx.astype(np.uint64)
    term = rng.integers(1, 50, G).astype(np.uint64)
    kind = rng.choice(5, G, p=[0.4, 0.15, 0.25, 0.15, 0.05])   # follower, candidate, leader, no leader yet, IS_NONE
    other = rng.integers(0, R, G).astype(np.uint64)
    other = np.where(rng.random(G) < 0.03, np.uint64(200), other)         # a SID index without a column
    idx = np.where((kind == 0) | (kind == 3), other, self_idx)
    lbit = ((kind == 0) | (kind == 2)).astype(np.uint64)
    term = np.where(kind == 4, 0, term).astype(np.uint64)
    hb.sid[:] = (term << np.uint64(9)) | (lbit << np.uint64(8)) | idx

    def beats(n, t, slot):
        dt = rng.integers(-2, 3, n)
        tt = np.maximum(t.astype(np.int64) + dt, 0).astype(np.uint64)
        return (tt << np.uint64(9)) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(8)) | slot

    quiet = rng.choice([0.1, 0.4, 0.95], G, p=[0.45, 0.30, 0.25])
    v = beats(G * R, np.repeat(term, R), np.tile(np.arange(R, dtype=np.uint64), G))
    v = np.where(rng.random(G * R) < np.repeat(quiet, R), 0, v)
    # the leader's own heartbeat is its SID (the common REARM case)
    sl = np.arange(G) * R + np.minimum(idx, R - 1).astype(np.int64)
    same = (rng.random(G) < 0.3) & (idx < R)
    v[sl[same]] = hb.sid[same]
    hb.hb[:] = v
    hb.vote_ack[:] = rng.integers(0, RING_LEN, G * R)
    hb.lr_step[:] = rng.integers(1, 7, G * R)
    hb.fail_count[:] = rng.integers(0, 4, G * R)
    hb.remote_end[:] = rng.integers(0, RING_LEN, G * R)
    hb.remote_commit[:] = rng.integers(0, RING_LEN, G * R)
    hb.apply_offsets[:] = rng.integers(0, RING_LEN, G * R)
    lat = np.where(rng.random(G) < 0.2, beats(G, term, idx) | np.uint64(1 << 9), 0)
    mode = rng.choice(4, G, p=[0.1, 0.45, 0.25, 0.2]) if explicit else None
    io = hb_io(G, R, mode=mode, latest_hb=lat, leader_failed=rng.integers(0, 2, G),
               send_flag=rng.integers(0, 2, G * R))
    return hb, io


def _clone(pkg, hb):
    c = pkg.batch.HostBatch(hb.G, hb.R, hb.stride, fields=list(hb.arrays))
    c.ring[:] = hb.ring
    for k, v in hb.arrays.items():
        c.arrays[k][:] = v
    return c


def _copy_io(io):
    return {k: (None if v is None else v.copy()) for k, v in io.items()}


@pytest.mark.parametrize("explicit", [True, False])
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("G", [g for g in GS if g >= 257])
def test_random_batches_hit_every_outcome(pkg, orc, G, R, explicit):
    """the histogram the GPU tests assert before they compare"""
    hb, io = random_hb_case(orc, G, R, explicit)
    before = _clone(pkg, hb)
    re_hb(hb, io)
    want = EXPLICIT_OUTCOMES if explicit else DERIVED_OUTCOMES
    assert set(np.unique(io["outcome"]).tolist()) == want, np.bincount(io["outcome"], minlength=12)
    # the restatement writes only what the reference writes
    for k in HB_UNCHANGED:
        assert np.array_equal(hb.arrays[k], before.arrays[k]), k
    assert np.array_equal(hb.ring, before.ring)
    cleared = (before.hb != 0) & (hb.hb == 0)
    assert cleared.any() and ((hb.hb == before.hb) | cleared).all()


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    assert torch.cuda.is_available()
    e = pkg.Engine(0)
    yield e
    e.close()


def _shift(t, torch, off):
    """the same bytes at a base `off` bytes past an allocation's start"""
    buf = torch.zeros(t.numel() + 16, dtype=torch.uint8, device=t.device)
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return v


def _device(pkg, hb, image, misalign, ring_len=RING_LEN):
    """hb on the device: state rows or dare_log_t images; misalign: hb and
    vote_ack 8 B, the byte rows 1 B past a 16-B boundary"""
    import torch
    if image:
        db = pkg.batch.LogImageBatch(hb.G, hb.R, ring_len)
        db.fill_from(hb)
        cols = db.cols.arrays
    else:
        db = pkg.batch.DeviceBatch(hb.G, hb.R, hb.stride)
        db.upload(hb)
        cols = db.arrays
    if misalign:
        for k, off in (("hb", 8), ("vote_ack", 8), ("lr_step", 1), ("fail_count", 1)):
            cols[k] = _shift(cols[k], torch, off)
            assert cols[k].data_ptr() % 16 == off
    return db


def _dev_io(io, misalign):
    import torch
    d = {}
    for k, v in io.items():
        if v is None:
            d[k] = None
            continue
        t = torch.from_numpy(v.view(np.uint8).copy()).cuda()
        d[k] = _shift(t, torch, 1) if misalign and v.dtype == np.uint8 else t
    return d


def _host_io(d, like):
    return {k: (None if v is None else v.cpu().numpy().view(like[k].dtype)) for k, v in d.items()}


def _cmp_batch(db, hb, image, written, unchanged):
    for k in written + unchanged:
        got = db.download(k)
        if k == "state":
            for f in ("head", "apply", "commit", "end", "tail", "len"):
                assert np.array_equal(got[f], hb.state[f]), f
            assert got["cid"].tobytes() == hb.state["cid"].tobytes(), "cid"
        else:
            assert np.array_equal(got, hb.arrays[k]), k
    ring = db.download("ring")
    want = hb.ring.reshape(hb.G, hb.stride)[:, :ring.shape[1]] if image else hb.ring
    assert np.array_equal(ring, want), "ring"


def _run_hb(pkg, eng, hb0, io0, want_hb, want_io, impl, image, misalign):
    db = _device(pkg, hb0, image, misalign)
    d = _dev_io(io0, misalign)
    b = db.struct()
    b.flags |= impl
    before = eng.stats()[pkg.abi.STAT_CORRUPT]
    eng.hb_tick(db, d, bstruct=b)
    got = _host_io(d, io0)
    for k in HB_OUT:
        assert np.array_equal(got[k], want_io[k]), (k, impl, image, misalign)
    _cmp_batch(db, want_hb, image, HB_WRITTEN, HB_UNCHANGED)
    assert eng.stats()[pkg.abi.STAT_CORRUPT] == before          # no compare-and-swap failed


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("G", GS)
def test_gpu_hb_random_batches(pkg, orc, eng, G, R):
    """apus_hb_batch against the restatement: the default and the lane form,
    explicit and derived modes, state rows and (G <= 65) log images, aligned
    and misaligned column bases -- every output, every column written in
    place, and the columns and ring bytes that must stay as they were"""
    abi = pkg.abi
    for explicit in (True, False):
        hb0, io0 = random_hb_case(orc, G, R, explicit)
        want_hb, want_io = _clone(pkg, hb0), _copy_io(io0)
        re_hb(want_hb, want_io)
        if G >= 257:
            want = EXPLICIT_OUTCOMES if explicit else DERIVED_OUTCOMES
            assert set(np.unique(want_io["outcome"]).tolist()) == want
        for impl in (0, abi.BATCH_LANE_IMPL):
            for image in ((False, True) if G <= 65 else (False,)):
                for misalign in (False, True):
                    _run_hb(pkg, eng, hb0, io0, want_hb, want_io, impl, image, misalign)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [0, 1])
def test_gpu_start_election(pkg, orc, eng, impl):
    """apus_start_election_batch for the due groups alone; a NULL send_flag
    leaves the other rows as the restatement writes them"""
    G, R = 321, 7
    hb0, _ = random_hb_case(orc, G, R, False, seed=1)
    rng = np.random.default_rng(5)
    io0 = {"due": (rng.random(G) < 0.5).astype(np.uint8), "send_flag": rng.integers(0, 2, G * R).astype(np.uint8),
           "outcome": np.zeros(G, np.uint8)}
    want_hb, want_io = _clone(pkg, hb0), _copy_io(io0)
    re_elect(want_hb, want_io)
    assert {IDLE, ELECTION} == set(np.unique(want_io["outcome"]).tolist())
    for null_flag in (False, True):
        db = _device(pkg, hb0, False, False)
        d = _dev_io(io0, False)
        if null_flag:
            d["send_flag"] = None
        b = db.struct()
        b.flags |= impl
        eng.start_election(db, d, bstruct=b)
        got = _host_io(d, io0)
        assert np.array_equal(got["outcome"], want_io["outcome"])
        if not null_flag:
            assert np.array_equal(got["send_flag"], want_io["send_flag"])
        _cmp_batch(db, want_hb, False, HB_WRITTEN, HB_UNCHANGED)


@pytest.mark.gpu
def test_gpu_hb_rows_landed_from_another_stream(pkg, orc, eng):
    """the heartbeat rows written by a copy on a second stream (standing in
    for the NIC), ordered by an event before the call"""
    import torch
    G, R = 513, 5
    hb0, io0 = random_hb_case(orc, G, R, True, seed=2)
    want_hb, want_io = _clone(pkg, hb0), _copy_io(io0)
    re_hb(want_hb, want_io)
    silent = _clone(pkg, hb0)
    silent.hb[:] = 0
    db = _device(pkg, silent, False, False)
    rows = torch.from_numpy(hb0.hb.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    nic = torch.cuda.Stream()
    with torch.cuda.stream(nic):
        db.arrays["hb"].copy_(rows)
        landed = torch.cuda.Event()
        landed.record(nic)
    torch.cuda.current_stream().wait_event(landed)
    d = _dev_io(io0, False)
    eng.hb_tick(db, d)
    got = _host_io(d, io0)
    for k in HB_OUT:
        assert np.array_equal(got[k], want_io[k]), k
    _cmp_batch(db, want_hb, False, HB_WRITTEN, HB_UNCHANGED)


# ------------------------------------------------------ the failure check
FAIL_CASES = {
    "wraps": dict(G=384, R=5, gen=dict(seed=411, n_entries=6, n_history=10, len_min=0, len_max=30, ring_len=1700,
                                       type_mix=True, cid_mix=True, self_random=True)),
    "c2_like": dict(G=300, R=3, gen=dict(seed=412, n_entries=8, n_history=8, len_min=64, len_max=64, ring_len=16384,
                                         self_random=True)),
    "wide": dict(G=257, R=7, gen=dict(seed=413, n_entries=10, n_history=14, len_min=0, len_max=90, ring_len=4000,
                                      type_mix=True, cid_mix=True, self_random=True)),
}
FAIL_WRITTEN = ("state", "prev_head")
FAIL_UNCHANGED = ("fail_count", "sid", "hb", "vote_ack", "lr_step", "remote_end", "remote_commit", "apply_offsets")
FAIL_OUT = ("req_id", "clt_id", "action", "connections", "removed", "cfg_idx")


def fail_case(pkg, orc, name):
    """rings from the trace generator at several fills (wrapping, full logs,
    unknown tails), fail_count around PERMANENT_FAILURE, leaders and
    followers, and groups whose end lies beyond len (REFUSED)"""
    c = FAIL_CASES[name]
    G, R = c["G"], c["R"]
    hb = orc.host_batch(G, R, c["gen"]["ring_len"])
    orc.gen(hb, pkg.batch.gen_cfg(**c["gen"]))
    rng = np.random.default_rng(c["gen"]["seed"])
    st = hb.state
    lead = rng.random(G) < 0.6
    term = rng.integers(1, 50, G).astype(np.uint64)
    idx = np.where(lead, hb.self_idx, (hb.self_idx.astype(np.int64) + 1) % R).astype(np.uint64)
    hb.sid[:] = (term << np.uint64(9)) | (np.uint64(1) << np.uint64(8)) | idx
    st["cid"]["state"] = np.where(rng.random(G) < 0.6, STABLE, st["cid"]["state"])
    hb.fail_count[:] = rng.choice(4, G * R, p=[0.7, 0.1, 0.1, 0.1])
    st["head"] = np.where(rng.random(G) < 0.1, st["end"], st["head"])              # full logs: the append returns 0
    st["tail"] = np.where(rng.random(G) < 0.15, st["len"], st["tail"])             # log_get_tail
    st["end"] = np.where(rng.random(G) < 0.1, st["len"] + np.uint64(8), st["end"])  # REFUSED where an append is due
    hb.prev_head[:] = rng.random(G) < 0.3
    io = fail_io(G, req_id=rng.integers(1, 1 << 20, G), clt_id=rng.integers(1, 1 << 16, G))
    return hb, io


@pytest.mark.parametrize("name", list(FAIL_CASES))
def test_failure_check_cases_hit_every_action(pkg, orc, name):
    hb, io = fail_case(pkg, orc, name)
    before = _clone(pkg, hb)
    refused = re_check_failure_count(pkg, orc, hb, io)
    assert set(np.unique(io["action"]).tolist()) == {F_NONE, F_SHUTDOWN, F_REMOVED, F_REFUSED}
    assert refused == int((io["action"] == F_REFUSED).sum()) > 0
    rem = io["action"] == F_REMOVED
    assert (io["cfg_idx"][rem] == 0).any() and (io["cfg_idx"][rem] != 0).any()     # full logs and appends
    assert (io["cfg_idx"][~rem] == 0).all()
    # only REMOVED groups changed
    same = hb.state[~rem].tobytes() == before.state[~rem].tobytes()
    assert same and np.array_equal(hb.ring.reshape(hb.G, -1)[~rem], before.ring.reshape(hb.G, -1)[~rem])


@pytest.mark.gpu
@pytest.mark.parametrize("name,image", [("wraps", False), ("wraps", True), ("c2_like", False), ("wide", False),
                                        ("wide", True)])
def test_gpu_failure_check(pkg, orc, eng, name, image):
    """apus_failure_check_batch against the restatement plus orc.append: ring
    bytes, state, cid, req_id / clt_id, the outputs, the REFUSED count (state
    rows, and dare_log_t images for the two small ring lengths)"""
    hb, io0 = fail_case(pkg, orc, name)
    db = _device(pkg, hb, image, False, FAIL_CASES[name]["gen"]["ring_len"])
    d = _dev_io(io0, False)
    before = eng.stats()[pkg.abi.STAT_CORRUPT]
    eng.check_failure_count(db, d)
    got = _host_io(d, io0)
    want_io = _copy_io(io0)
    refused = re_check_failure_count(pkg, orc, hb, want_io)
    for k in FAIL_OUT:
        assert np.array_equal(got[k], want_io[k]), k
    _cmp_batch(db, hb, image, FAIL_WRITTEN, FAIL_UNCHANGED)
    assert eng.stats()[pkg.abi.STAT_CORRUPT] - before == refused > 0


# -------------------------------------------------------------- the cycle
@pytest.mark.gpu
def test_gpu_election_cycle(pkg, orc, eng):
    """heartbeat timeout -> election start -> tally -> win -> failure check ->
    heartbeat send, every step against the restatement and the oracle"""
    from test_apply import build as apply_build
    abi = pkg.abi
    G, R = 256, 5
    case = dict(G=G, R=R, gen=dict(seed=421, n_entries=6, n_history=6, len_min=0, len_max=60, ring_len=4000,
                                   type_mix=True, cid_mix=True))
    hb, cid_offset, cid_idx = apply_build(pkg, orc, "cycle", case)
    rng = np.random.default_rng(421)
    st = hb.state
    st["cid"]["state"] = np.where(rng.random(G) < 0.5, STABLE, st["cid"]["state"])
    term = rng.integers(1, 50, G).astype(np.uint64)
    leader = (hb.self_idx.astype(np.uint64) + np.uint64(1)) % np.uint64(R)
    hb.sid[:] = (term << np.uint64(9)) | (np.uint64(1) << np.uint64(8)) | leader     # followers of a silent leader
    hb.hb[:] = 0
    hb.fail_count[:] = 0
    db = pkg.batch.DeviceBatch(G, R, hb.stride)
    db.upload(hb)
    keys = HB_WRITTEN + ("remote_commit", "apply_offsets", "prev_head", "fail_count")

    def same(step):
        for k in keys:
            assert np.array_equal(db.download(k).view(np.uint8), hb.arrays[k].view(np.uint8)), (step, k)
        assert np.array_equal(db.download("ring"), hb.ring), (step, "ring")

    def tick(step):
        io = hb_io(G, R)
        d = _dev_io(io, False)
        eng.hb_tick(db, d)
        re_hb(hb, io)
        got = _host_io(d, io)
        for k in HB_OUT:
            assert np.array_equal(got[k], io[k]), (step, k)
        same(step)
        return io

    # 1. all-zero heartbeats: every member times out and starts an election
    io = tick(1)
    member = hb.self_idx < np.array([group_size(c) for c in st["cid"]])
    assert member.sum() > G // 2 and (io["outcome"][member] == ELECTION).all()
    assert (io["outcome"][~member] == NOT_MEMBER).all()
    # 2. the peers' votes
    votes = (rng.random((G, R)) < 0.7) & (np.arange(R)[None, :] != hb.self_idx[:, None])
    ack = np.where(votes, st["commit"][:, None], hb.vote_ack.reshape(G, R)).astype(np.uint64).reshape(-1)
    hb.vote_ack[:] = ack
    db.arrays["vote_ack"].copy_(db.torch.from_numpy(ack.view(np.uint8)))
    # 3. the tally and the win
    vo = eng.poll_vote_count(db)
    v = orc.vote(hb)
    for k in ("won", "new_commit"):
        assert np.array_equal(vo[k].cpu().numpy().view(v[k].dtype), v[k]), k
    wio = orc.win_io(G, v["won"], v["voters"], v["new_commit"], cid_offset, cid_idx)
    got = eng.become_leader(db, dict(wio))
    orc.vote_win(hb, wio)
    for k in ("outcome", "req_id", "clt_id", "last_write_csm_idx", "departed"):
        assert np.array_equal(got[k], wio[k]), k
    same(3)
    winner = (wio["outcome"] >= abi.WIN_CONFIG) & (wio["outcome"] <= abi.WIN_UNDEFINED)
    assert winner.sum() > 20
    assert all(is_leader(int(s), int(i)) for s, i in zip(hb.sid[winner], hb.self_idx[winner]))
    # 4. one failed follower: removed by the winners whose cid is STABLE
    failed = (hb.self_idx.astype(np.int64) + 1) % R
    hb.fail_count.reshape(G, R)[np.arange(G), failed] = PERMANENT_FAILURE
    db.arrays["fail_count"].copy_(db.torch.from_numpy(hb.fail_count))
    fio = fail_io(G, req_id=wio["req_id"], clt_id=wio["clt_id"])
    d = _dev_io(fio, False)
    eng.check_failure_count(db, d)
    re_check_failure_count(pkg, orc, hb, fio)
    got = _host_io(d, fio)
    for k in FAIL_OUT:
        assert np.array_equal(got[k], fio[k]), k
    same(4)
    removed = fio["action"] == F_REMOVED
    assert removed.sum() > 5 and not (removed & ~winner).any()
    assert (st["cid"]["state"][removed] == STABLE).all()
    assert (fio["action"][~winner] != F_REMOVED).all()
    # 5. the winners send heartbeats
    io = tick(5)
    assert (io["outcome"][winner] == SEND).all()
