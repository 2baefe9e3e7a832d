"""The opt-in CRC-32C entry digest (apus_crc32c_batch, APUS_COMMIT_CRC32C).

digest[g] is the CRC-32C of RFC 3720 (Castagnoli, reflected 0x82F63B78, init
and final XOR 0xFFFFFFFF) over the byte string the Adler-32 digest covers: the
concatenated spans of the entries the walk chain visits from commit to end,
bytes 27..47 of each read as zero.  The reference is this file's own
table-driven CRC-32C (pinned with the RFC's known answers), vectorised over
groups, on a restatement of the image rule that reproduces the oracle's
Adler-32 through zlib.adler32.  Every comparison is exact.
"""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest
from test_gpu_parity import CFGS, RS, _malformed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINTS = {"wave": 0, "lane": 0x1, "short": 0x2, "var": 0x8}      # BATCH_LANE_IMPL / SHORT_WALKS / VAR_LEN

_T = np.zeros(256, np.uint32)
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _T[_i] = _c


def crc32c_many(msgs):
    """CRC-32C of each byte string, one table step per byte position"""
    n = len(msgs)
    lens = np.array([len(m) for m in msgs], np.int64)
    order = np.argsort(-lens, kind="stable")
    width = int(lens.max()) if n else 0
    buf = np.zeros((n, width), np.uint8)
    for k, j in enumerate(order):
        buf[k, :lens[j]] = np.frombuffer(msgs[j], np.uint8)
    sl = lens[order]
    c = np.full(n, 0xFFFFFFFF, np.uint32)
    live = n
    for i in range(width):
        while live and sl[live - 1] <= i:
            live -= 1
        v = c[:live]
        c[:live] = _T[(v ^ buf[:live, i]) & 0xFF] ^ (v >> 8)
    out = np.empty(n, np.uint32)
    out[order] = c ^ np.uint32(0xFFFFFFFF)
    return out


def crc32c(data):
    return int(crc32c_many([bytes(data)])[0])


def _chain(hb, g):
    """(image, [(offset, length)]) of group g: the image rule of
    tests/test_checksum.py::_images; a group with commit or end beyond len
    covers nothing"""
    ring = hb.group_ring(g)
    s = hb.state[g]
    ln, end, m = int(s["len"]), int(s["end"]), int(s["commit"])
    if m > ln or end > ln or ln > hb.stride:
        return b"", []

    def dist(o):
        return 0 if end == ln else (end - o if end >= o else ln - (o - end))
    out, ents, steps = bytearray(), [], 0
    while dist(m) and steps < ln // 64 + 4:
        steps += 1
        if ln - m < 64:
            m = 0
        t = int(ring[m + 26])
        clen = int(ring[m + 48]) | (int(ring[m + 49]) << 8)
        el = 64 if t in (0, 2, 3) else 64 + clen
        if ln - m < el:
            m = 0
            continue
        out += bytes(ring[m:m + 27]) + bytes(21) + bytes(ring[m + 48:m + el])
        ents.append((m, el))
        m += el
    return bytes(out), ents


def _want(hb, groups=None):
    return crc32c_many([_chain(hb, g)[0] for g in (range(hb.G) if groups is None else groups)])


# ------------------------------------------------------------------- CPU
def test_crc32c_known_answers():
    """RFC 3720 B.4"""
    for data, want in [(b"123456789", 0xE3069283), (bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43),
                       (bytes(range(32)), 0x46DD794E), (bytes(range(31, -1, -1)), 0x113FDB5C), (b"", 0)]:
        assert crc32c(data) == want
    msgs = [b"123456789", b"", bytes(32), bytes(range(32))]
    assert list(crc32c_many(msgs)) == [0xE3069283, 0, 0x8A9136AA, 0x46DD794E]


def test_image_rule_is_the_oracles(pkg, orc):
    """the restated image reproduces the oracle's Adler-32, malformed rings included"""
    kw = CFGS["mixed_small"]
    hb = orc.host_batch(256, RS["mixed_small"], kw["ring_len"])
    orc.gen(hb, pkg.batch.gen_cfg(**kw))
    for h in (hb, _malformed(pkg, orc, 512, 4105, False)):
        ref = orc.commit(h, pkg.abi.COMMIT_CHECKSUM)
        for g in range(h.G):
            assert ref["digest"][g] == zlib.adler32(_chain(h, g)[0]), g


def test_crc32c_flag_in_header_and_mirror(pkg):
    text = open(os.path.join(ROOT, "include", "apus_gpu.h")).read()
    m = re.search(r"^#define\s+APUS_COMMIT_CRC32C\s+(0x[0-9a-fA-F]+)u", text, re.M)
    assert m and int(m.group(1), 0) == 0x800
    assert pkg.abi.COMMIT_CRC32C == 0x800


def test_crc32c_batch_exported_and_refuses_null(pkg):
    abi = pkg.abi
    nm = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT apus_crc32c_batch\b", nm)
    assert "apus_crc32c_batch" in [n for n, _, _ in abi.SIGNATURES]
    lib = abi.load_library()
    assert lib.apus_crc32c_batch(None, None, None, None) == abi.APUS_ERROR
    b = abi.Batch(n_groups=0, n_replicas=3)
    assert lib.apus_crc32c_batch(None, C.byref(b), None, None) == abi.APUS_ERROR


# ------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def eng(pkg):
    import torch
    assert torch.cuda.is_available()
    e = pkg.Engine(0)
    yield e
    e.close()


_CACHE = {}


def _host(pkg, orc, name, G):
    """the oracle-generated batch of CFGS[name] and its expected digests, made once"""
    if (name, G) not in _CACHE:
        kw = CFGS[name]
        hb = orc.host_batch(G, RS[name], kw["ring_len"])
        orc.gen(hb, pkg.batch.gen_cfg(**kw))
        _CACHE[name, G] = (hb, _want(hb))
    return _CACHE[name, G]


def _device(pkg, hb):
    db = pkg.batch.DeviceBatch(hb.G, hb.R, hb.stride)
    db.upload(hb)
    return db


def _digest(eng, db, hint=0, b=None):
    import torch
    b = db.struct() if b is None else b
    b.flags |= hint
    d = eng.crc32c(db, bstruct=b)
    torch.cuda.synchronize()
    return d.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


PARITY_G = {"c3_var": 128, "multiwin": 512}


@pytest.mark.gpu
@pytest.mark.parametrize("hint", list(HINTS))
@pytest.mark.parametrize("name", list(CFGS))
def test_crc32c_batch_parity(pkg, orc, eng, name, hint):
    hb, want = _host(pkg, orc, name, PARITY_G.get(name, 1024))
    db = _device(pkg, hb)
    before = eng.stats()
    assert np.array_equal(_digest(eng, db, HINTS[hint]), want)
    assert np.array_equal(eng.stats(), before)              # the call counts nothing
    eng.stats_reset()
    zero = eng.stats()
    assert np.array_equal(_digest(eng, db, HINTS[hint]), want)
    assert np.array_equal(eng.stats(), zero)


@pytest.mark.gpu
@pytest.mark.parametrize("hint", list(HINTS))
@pytest.mark.parametrize("name", ["c2_skew", "mixed_small", "wrap_aligned", "c5"])
def test_crc32c_commit_flag(pkg, orc, eng, name, hint):
    """APUS_COMMIT_CRC32C beside a whole commit call: the digest is the CRC,
    every other output and statistic is the call's without the flag and the
    oracle's"""
    import torch
    abi = pkg.abi
    hb, want = _host(pkg, orc, name, 1024)
    base = abi.COMMIT_WALK | abi.COMMIT_MEDIAN | abi.COMMIT_PRUNE | abi.COMMIT_NC | abi.COMMIT_LAST_IT
    M = 40
    runs = []
    for flags in (base | abi.COMMIT_CRC32C, base):
        db = _device(pkg, hb)
        b = db.struct()
        b.flags = HINTS[hint]
        eng.stats_reset()
        out = eng.update_remote_logs(db, flags, bstruct=b, nc_max=M)
        torch.cuda.synchronize()
        runs.append((out, eng.stats(), db.download("apply_offsets"), db.download("ring")))
    (oa, sa, apa, ra), (ob, sb, apb, rb) = runs
    assert np.array_equal(oa["digest"].cpu().numpy().view(np.uint32), want)
    assert "digest" not in ob
    for k in ob:
        if k != "nc_max":
            assert torch.equal(oa[k], ob[k]), k
    assert np.array_equal(sa, sb) and np.array_equal(apa, apb)
    assert np.array_equal(ra, hb.ring) and np.array_equal(rb, hb.ring)
    # ... and the oracle's
    ref = orc.commit(hb, abi.COMMIT_WALK | abi.COMMIT_MEDIAN)
    assert np.array_equal(_u64(oa["new_commit"]), ref["new_commit"])
    assert np.array_equal(oa["committed"].cpu().numpy(), ref["committed"])
    assert np.array_equal(oa["n_entries"].cpu().numpy().view(np.uint32), ref["n_entries"])
    assert np.array_equal(_u64(oa["median"]), ref["median"])
    rd, rl = orc.nc_build(hb, M)
    assert np.array_equal(oa["nc_len"].cpu().numpy().view(np.uint32), rl)
    got = oa["nc_dets"].cpu().numpy().view(np.uint64).reshape(hb.G, 3 * M)
    live = np.arange(3 * M)[None, :] < 3 * rl.astype(np.int64)[:, None]
    assert np.array_equal(np.where(live, got, 0), np.where(live, rd.reshape(hb.G, 3 * M), 0))
    assert np.array_equal(_u64(oa["last_idx_term"]).reshape(-1), orc.last_idx_term(hb))
    h2 = pkg.batch.HostBatch(hb.G, hb.R, hb.stride, fields=list(hb.arrays))     # orc.prune writes apply_offsets
    h2.ring[:] = hb.ring
    for k, v in hb.arrays.items():
        h2.arrays[k][:] = v
    rp, wm = orc.prune(h2)
    assert np.array_equal(_u64(oa["new_head"]), rp["new_head"])
    assert np.array_equal(oa["append_head"].cpu().numpy(), rp["append_head"])
    assert np.array_equal(_u64(oa["min_apply"]), rp["min_apply"])
    assert np.array_equal(apa, h2.apply_offsets)
    assert sa[abi.STAT_DECISIONS] == hb.G
    assert sa[abi.STAT_COMMITTED] == int(ref["n_entries"].sum())
    assert sa[abi.STAT_ADVANCED] == int((ref["committed"] == 1).sum())
    assert sa[abi.STAT_MIN_WATERMARK] == wm

    # the flag alone: no walk, the same digests, nothing else written
    db = _device(pkg, hb)
    b = db.struct()
    b.flags = HINTS[hint]
    eng.stats_reset()
    zero = eng.stats()
    out = eng.update_remote_logs(db, abi.COMMIT_CRC32C, bstruct=b)
    torch.cuda.synchronize()
    assert np.array_equal(out["digest"].cpu().numpy().view(np.uint32), want)
    assert not out["new_commit"].any() and not out["committed"].any() and not out["n_entries"].any()
    assert np.array_equal(eng.stats(), zero)

    # one digest array: refused beside the Adler-32 flag, and beside FORCE_PRUNE as that flag is
    for bad in (abi.COMMIT_CRC32C | abi.COMMIT_CHECKSUM, abi.COMMIT_WALK | abi.COMMIT_CRC32C | abi.COMMIT_CHECKSUM,
                abi.COMMIT_CRC32C | abi.COMMIT_FORCE_PRUNE):
        out = eng.alloc_commit_out(hb.G, bad | abi.COMMIT_MEDIAN)
        tensors = [v for v in out.values() if hasattr(v, "fill_")] + list(out["force"].values() if "force" in out else [])
        for t in tensors:
            t.view(torch.uint8).fill_(0x5A)
        o = eng.commit_struct(out)
        assert eng.lib.apus_commit_batch(eng.ctx, C.byref(b), C.byref(o), bad, eng._stream()) == abi.APUS_ERROR
        torch.cuda.synchronize()
        for t in tensors:
            assert bool((t.view(torch.uint8) == 0x5A).all())
        assert np.array_equal(eng.stats(), zero)


@pytest.mark.gpu
@pytest.mark.parametrize("hint", list(HINTS))
def test_crc32c_malformed_rings(pkg, orc, eng, hint):
    """chains that overshoot end, garbage headers, random commits: the wave
    form defers what it cannot settle to the exact form (its deferred list
    holds every group, so it cannot overflow); groups that cover nothing give 0"""
    if "bad" not in _CACHE:
        hb = _malformed(pkg, orc, 4096, 4105, False)
        st = hb.state
        L = int(st["len"][0])
        empty = {"commit": [7, 1001, 4000], "end": [8, 1002, 4001], "same": [9]}
        for g in empty["commit"]:
            st["commit"][g] = L + 16
        for g in empty["end"]:
            st["end"][g] = L + 1
        for g in empty["same"]:
            st["commit"][g] = st["end"][g] = 128
        _CACHE["bad"] = (hb, _want(hb), sum(empty.values(), []))
    hb, want, empty = _CACHE["bad"]
    assert not want[empty].any()
    db = _device(pkg, hb)
    assert np.array_equal(_digest(eng, db, HINTS[hint]), want)
    assert np.array_equal(db.download("ring"), hb.ring)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 63, 65, 3037])
@pytest.mark.parametrize("name", ["tiny_wrap", "c2"])
def test_crc32c_wave_edges(pkg, orc, eng, name, G):
    """fewer groups than a block's waves, one off a wave's 64, a ragged last block"""
    hb, want = _host(pkg, orc, name, G)
    assert np.array_equal(_digest(eng, _device(pkg, hb)), want)


@pytest.mark.gpu
def test_crc32c_rebased_ring_takes_the_exact_form(pkg, orc, eng):
    """a ring array that is not 16-B aligned is walked one lane per group: same digests"""
    import torch
    hb, want = _host(pkg, orc, "c2", 1024)
    db = _device(pkg, hb)
    moved = torch.zeros(db.ring.numel() + 16, dtype=torch.uint8, device=db.ring.device)
    moved[8:8 + db.ring.numel()] = db.ring
    b = db.struct()
    b.ring = moved.data_ptr() + 8
    assert b.ring % 16 == 8
    assert np.array_equal(_digest(eng, db, b=b), want)
    assert np.array_equal(_digest(eng, db), want)


@pytest.mark.gpu
@pytest.mark.parametrize("hint", list(HINTS))
def test_crc32c_log_image_batch(pkg, orc, eng, hint):
    """dare_log_t images (APUS_BATCH_LOG_IMAGE), built as tests/test_log_image.py builds them"""
    import torch
    kw = dict(seed=803, n_entries=12, n_history=3, len_min=0, len_max=100, ring_len=4096, type_mix=True,
              cid_mix=True, self_random=True, p_full_ack=0.6, straggler=True)
    if "img" not in _CACHE:
        hb = orc.host_batch(777, 5, kw["ring_len"])
        orc.gen(hb, pkg.batch.gen_cfg(**kw))
        _CACHE["img"] = (hb, _want(hb))
    hb, want = _CACHE["img"]
    img = pkg.batch.LogImageBatch(hb.G, hb.R, kw["ring_len"])
    img.fill_from(hb)
    b = img.struct()
    b.flags |= HINTS[hint]
    d = eng.crc32c(img, bstruct=b)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32), want)


@pytest.mark.gpu
def test_crc32c_sees_the_image_and_nothing_else(pkg, orc, eng):
    import torch
    hb, want = _host(pkg, orc, "c2", 512)
    db = _device(pkg, hb)
    rng = np.random.default_rng(77)
    # bytes 27..47 of every entry in [commit, end): the followers' writes
    host = hb.ring.copy()
    flip_at = np.zeros(hb.G, np.int64)
    for g in range(hb.G):
        ents = _chain(hb, g)[1]
        assert ents
        for m, _ in ents:
            host[g * hb.stride + m + 27:g * hb.stride + m + 48] = rng.integers(0, 256, 21)
        m, el = ents[rng.integers(0, len(ents))]
        k = int(rng.integers(0, el - 24))           # not the type or cmd.len: the chain stays as it is
        flip_at[g] = g * hb.stride + m + (k if k < 26 else k + 24)
    db.ring.copy_(torch.from_numpy(host))
    assert np.array_equal(_digest(eng, db), want)
    assert np.array_equal(_digest(eng, db, HINTS["lane"]), want)
    assert np.array_equal(db.download("ring"), host)            # the calls wrote no ring byte
    # one bit of one other image byte per group: CRC-32C detects every single-bit error
    host[flip_at] ^= (1 << rng.integers(0, 8, hb.G)).astype(np.uint8)
    h2 = pkg.batch.HostBatch(hb.G, hb.R, hb.stride, fields=list(hb.arrays))
    h2.ring[:] = host
    for k, v in hb.arrays.items():
        h2.arrays[k][:] = v
    want2 = _want(h2)
    assert (want2 != want).all()
    db.ring.copy_(torch.from_numpy(host))
    assert np.array_equal(_digest(eng, db), want2)
    assert np.array_equal(_digest(eng, db, HINTS["lane"]), want2)
    assert np.array_equal(db.download("ring"), host)
