"""GPU: everything a row shard writes - flags, offsets, the packed list, the answer block - held to tests/shard_model.py, a function of the
oracle's f32 scores and the segment plan, with no tolerance; bbq_merge_answers and bbq_replay_batch over the device's words held to the
model's status and the oracle's heap; the packed capacity's three regimes; two batches in flight; the multi-device handle's answers and
the three figures of its statistics that are functions of the model.  All shards live on device 0.

No query is left out of any comparison.  A flagged query is compared too: its flags, its empty list, {0 | unproven} and cut 0 - all but
the `entries listed` half of its slot 0 (shard_model's docstring says why).  Where the model is not exact (the flooding query of the
`inner` and `mid` floods) the invariants are asserted instead: a superset list, a cut at most the true one, entries exactly the own rows
above the device's own cut - and `unproven` both ways: set where a size test of the `ok` chain fails on the device's own list or the
subset scan finds more than k own rows above its cut (`inner`), clear with 0 < cut <= the true cut where it does not (`mid`).

tests/test_shard_model_cpu.py holds the model to brute force.  A BBQ_ERR_HIP from any call ends the whole pytest session
(test_gpu_mutation_walk.located)."""
import collections
import contextlib
import ctypes as C

import numpy as np
import pytest

import candidate_model as M
import orclib as O
import shard_model as S
from bbqlib import bbq_amd as B, capi
from test_gpu_fast_bound import bits32
from test_gpu_mutation_walk import located, refused

pytestmark = pytest.mark.gpu

GRID, TINY = S.grid_cases(), S.tiny_cases()
TALLY = collections.defaultdict(lambda: [0, 0, 0, 0])      # family -> [blocks compared, list entries compared, exact blocks, invariant-only blocks]
U32 = np.uint64(0xFFFFFFFF)
SUBSET = {}      # id(an inexact model) -> (the model, its subset scan, the first own row of the plan's last segment)


@pytest.fixture(scope="module", autouse=True)
def _tally():
    yield
    for name, (blocks, entries, exact, inv) in sorted(TALLY.items()):
        print("shard model: family %s: %d (shard, query, k) scans compared, %d list entries, %d exact blocks, %d invariant-only" % (name, blocks, entries, exact, inv))


@contextlib.contextmanager
def opened(data, shards, fam, opts=S.OPTS):
    """one index per shard, on device 0, under the recipe's options"""
    ixs = []
    try:
        for sh in shards:
            pil = len(sh.pilot) > 0
            ix = B.Index(data.codes[sh.r0:sh.r1], data.corr[sh.r0:sh.r1], fam.dim, M.CDP, index_bits=fam.index_bits, row_base=sh.r0,
                         pilot_codes=data.codes[sh.pilot] if pil else None, pilot_corr=data.corr[sh.pilot] if pil else None)
            ixs.append(ix)
            for name, value in opts.items():
                ix.set_option(name, value)
        yield ixs
    finally:
        for ix in ixs:
            ix.close()


class Buffers:
    def __init__(self, nq, cap, k, answers, fill=0):
        import torch
        self.nq, self.cap, self.stride = nq, cap, k + 3
        self.packed = torch.full((cap,), fill, dtype=torch.int64, device="cuda")
        self.off = torch.full((nq + 1,), fill, dtype=torch.int64, device="cuda")
        self.flags = torch.full((nq,), fill, dtype=torch.int32, device="cuda")
        self.ans = torch.full((nq * self.stride,), fill, dtype=torch.int64, device="cuda") if answers else None

    def begin(self, ix, qq, qc, qb, sim, k):
        ix.shard_scan_begin(qq, qc, qb, sim, k, self.packed.data_ptr(), self.cap, self.off.data_ptr(), self.flags.data_ptr(),
                            self.ans.data_ptr() if self.ans is not None else None, self.stride if self.ans is not None else 0)

    def read(self, total):
        """(flags, offsets, packed[:total], blocks [nq, k + 3] or None) on the host"""
        blocks = self.ans.cpu().numpy().view(np.uint64).reshape(self.nq, self.stride) if self.ans is not None else None
        return self.flags.cpu().numpy(), self.off.cpu().numpy(), self.packed[:total].cpu().numpy().view(np.uint64), blocks


def generous(ix, sh, nq, k):
    return nq * max(int(ix.shard_list_cap(k)), sh.r1 - sh.r0 + 1024)


def scan(ix, sh, data, qs, fam, sim, k, answers=True, cap=None, fill=-1):
    """begin + wait of the queries `qs` on one shard: (flags, offsets, packed, blocks)"""
    buf = Buffers(len(qs), cap or generous(ix, sh, len(qs), k), k, answers, fill)
    buf.begin(ix, data.qq[qs], data.qc[qs], fam.query_bits, sim, k)
    total = ix.shard_scan_wait()
    out = buf.read(total)
    assert total == int(out[1][-1]), "the total bbq_shard_scan_wait reports is not offsets[n_queries]"
    return out


def models_of(ix, sh, data, qs, fam, k, answers, opts=S.OPTS):
    kd = k + 1 if answers else k
    cap = int(ix.shard_list_cap(k))
    if answers or k > S.K_FINAL_SELECT_MAX:      # (a lists-only scan of k <= 1024 runs the rank-k plan: bbq_shard_list_cap sizes for rank k + 1)
        segs = S.shard_segments(len(sh.pilot), sh.r1 - sh.r0, kd, opts["first_segment_rows"], opts["segment_growth"])
        assert cap == S.planned_list_cap(segs, kd), "bbq_shard_list_cap(%d) = %d, the plan's %d" % (k, cap, S.planned_list_cap(segs, kd))
    ms = [S.scan_model(*S.shard_scores(data, sh, q), sh.r0, k, answers, opts, cap, fam) for q in qs]
    for q, m in zip(qs, ms):
        if not m.exact:      # what the keys that fit give (scan_model's `subset`): kept beside the model, which holds the true statistics
            SUBSET[id(m)] = (m, S.scan_model(*S.shard_scores(data, sh, q), sh.r0, k, answers, opts, cap, fam, subset=True),
                             S.shard_segments(len(sh.pilot), sh.r1 - sh.r0, kd, opts["first_segment_rows"], opts["segment_growth"])[-1].first)
    return ms, cap


def check(got, models, list_cap, packed_cap, k, answers, fam, msg):
    """ONE batch on ONE shard against its models: every word"""
    flags, off, packed, blocks = got
    exact = [m.exact for m in models]
    bad = []
    if all(exact):
        wflags, woff, wtotal, oom = S.pack_model([len(m.rows) for m in models], [m.flags for m in models], list_cap, packed_cap)
        assert not oom
        if flags.tolist() != wflags.tolist():
            bad.append("FLAGS %s, the model's %s (%s)" % (flags.tolist(), wflags.tolist(), [m.reasons for m in models]))
        if off.tolist() != woff.tolist():
            bad.append("OFFSETS: lengths %s, the model's %s" % (np.diff(off).tolist(), np.diff(woff).tolist()))
    else:      # a batch with an inexact model: its exact queries one by one (every such batch has room for all its lists: no squeeze)
        assert int(off[-1]) <= packed_cap and off[0] == 0
        for q, m in enumerate(models):
            if m.exact and (flags[q] != m.flags or off[q + 1] - off[q] != (0 if m.flags else len(m.rows))):
                bad.append("FLAGS / LENGTH of query %d: %d / %d, the model's %d / %d (%s)" % (q, flags[q], off[q + 1] - off[q], m.flags, len(m.rows), m.reasons))
    for q, m in enumerate(models):
        mine = packed[off[q]:off[q + 1]] if off[q + 1] <= len(packed) else np.zeros(0, np.uint64)
        want = (m.rows.astype(np.uint64) << np.uint64(32)) | m.bits.astype(np.uint64)
        TALLY[fam.name][0] += 1
        if m.exact:
            if flags[q] == 0 and (len(mine) != len(want) or (mine != want).any()):      # the model's set, the f32 bits, ascending by global row
                bad.append("LIST of query %d: %d entries, the model's %d; first difference at %s" % (
                    q, len(mine), len(want), np.flatnonzero(mine[:min(len(mine), len(want))] != want[:min(len(mine), len(want))])[:1]))
            if flags[q] != 0 and len(mine) != 0:
                bad.append("LIST of query %d: a flagged query carries %d entries" % (q, len(mine)))
            TALLY[fam.name][1] += len(mine)
        else:
            rows = (mine >> np.uint64(32)).astype(np.int64)
            inside = len(rows) == 0 or (rows.min() >= m.row_base and rows.max() < m.row_base + len(m.own))
            right = inside and ((mine & U32).astype(np.uint32) == m.own[rows - m.row_base].view(np.uint32)).all()
            if flags[q] != m.flags or (np.diff(rows) <= 0).any() or not right or (m.flags and len(rows)) or (not m.flags and not set(m.rows.tolist()) <= set(rows.tolist())):
                bad.append("LIST of query %d (invariants): flags %d, ascending %s, own rows with their bits %s, superset of the true thresholds' list %s" % (
                    q, flags[q], (np.diff(rows) > 0).all(), right, set(m.rows.tolist()) <= set(rows.tolist())))
            TALLY[fam.name][1] += len(mine)
        if not answers:
            continue
        blk = blocks[q]
        listed, bflags, cnt, unproven, cut = S.header(blk)
        if m.exact:
            TALLY[fam.name][2] += 1
            w = m.block
            same = (blk[1:len(w)] == w[1:]).all() and bflags == m.flags and (m.flags != 0 or listed == S.header(w)[0])
            if not same:
                bad.append("BLOCK of query %d: header %s entries %s..., the model's %s %s... (%s, branch %s)" % (
                    q, S.header(blk), blk[3:6], S.header(w), w[3:6], m.why_not, m.branch))
        else:
            TALLY[fam.name][3] += 1
            _, dev, last_first = SUBSET[id(m)]
            print("shard model: invariant-only block, %s query %d: header %s; the true cut %d, the subset scan's %d (%s)" % (
                msg, q, S.header(blk), m.cut, dev.cut, dev.why_not))
            if bflags != m.flags or cnt > k or cut > m.cut or (bflags and not unproven) or (not bflags and listed != len(mine)) or (unproven and (cnt or cut)):
                bad.append("BLOCK of query %d (invariants): header %s, the true cut %d" % (q, S.header(blk), m.cut))
            if not bflags:
                # `unproven` both ways.  The two size tests of the `ok` chain from the device's OWN list; behind them only "n_sel <= k2"
                # is left, which the subset scan decides
                m_last = int(((mine >> np.uint64(32)).astype(np.int64) >= m.row_base + last_first).sum())
                sizes_fail = listed > m.room or m_last > S.KEY_CAP - m.tcount
                if sizes_fail and not unproven:
                    bad.append("BLOCK of query %d: proven with %d entries listed (room %d), %d of the last segment beside %d running keys" % (q, listed, m.room, m_last, m.tcount))
                if not sizes_fail and bool(unproven) != (not dev.ok):
                    bad.append("BLOCK of query %d: unproven %d; the size tests pass and the subset scan says %s" % (q, unproven, dev.why_not or "proven"))
                if dev.ok and not (unproven == 0 and 0 < cut <= m.cut and cut == dev.cut):
                    bad.append("BLOCK of query %d: a proven block with 0 < cut <= %d expected (the subset scan's cut %d): header %s" % (q, m.cut, dev.cut, S.header(blk)))
            if not unproven:
                ents = blk[3:3 + cnt]
                above = np.flatnonzero(M.keys_of(m.own) > cut) + m.row_base      # the own rows above the device's cut
                erows = (ents >> np.uint64(32)).astype(np.int64)
                ekeys = M.keys_of((ents & U32).astype(np.uint32).view(np.float32))
                if sorted(erows.tolist()) != above.tolist() or (np.diff(ekeys.astype(np.int64)) > 0).any() or \
                        ((ents & U32).astype(np.uint32) != m.own[erows - m.row_base].view(np.uint32)).any():
                    bad.append("BLOCK of query %d (invariants): the entries are not the own rows above its cut, descending" % q)
    assert not bad, "%s, k %d, %s\n%s" % (msg, k, "answers" if answers else "lists only", "\n".join(bad))


def end_to_end(data, shards, results, models, k, msg, qs):
    """merge all shards' blocks, replay the status-1 queries from the packed lists: the model's status, the oracle's answers"""
    nq = len(qs)
    idx, sc, cnt, status = B.merge_answers([r[3] for r in results], nq, data.n, k, 2)
    ri, rs, rc = B.replay_batch([r[2] for r in results], [r[1] for r in results], nq, data.n, k, 2)
    bad = []
    for i, q in enumerate(qs):
        per_shard = [ms[i] for ms in models]
        if all(m.exact for m in per_shard):
            want = S.merge_model([m.block for m in per_shard], data.scores[q], k)
            if status[i] != want:
                bad.append("STATUS of query %d: %d, the model's %d" % (i, status[i], want))
        flagged = any(m.flags for m in per_shard)
        if (status[i] == 2) != flagged:
            bad.append("STATUS of query %d: %d, flagged by the model: %s" % (i, status[i], flagged))
        if flagged:
            continue
        oi, osc = O.heap_topk(data.scores[q], k)
        if status[i] == 0 and (cnt[i] != len(oi) or (idx[i, :cnt[i]] != oi).any() or (bits32(sc[i, :cnt[i]]) != bits32(osc)).any()):
            bad.append("MERGED ANSWER of query %d: rows %s, the oracle's %s" % (i, idx[i, :cnt[i]][:12], oi[:12]))
        if rc[i] != len(oi) or (ri[i, :rc[i]] != oi).any() or (bits32(rs[i, :rc[i]]) != bits32(osc)).any():
            bad.append("REPLAYED ANSWER of query %d: rows %s, the oracle's %s" % (i, ri[i, :rc[i]][:12], oi[:12]))
    assert not bad, "%s, k %d\n%s" % (msg, k, "\n".join(bad))
    return status


def run_case(case, ks_answers, ks_lists=()):
    data = S.case_data(case)
    fam, qs = case.fam, list(range(len(data.scores)))
    with located(case.name), opened(data, data.shards, fam) as ixs:
        for k in ks_answers:
            results, models = [], []
            for sh, ix in zip(data.shards, ixs):
                ms, cap = models_of(ix, sh, data, qs, fam, k, True)
                got = scan(ix, sh, data, qs, fam, case.sim, k)
                check(got, ms, cap, generous(ix, sh, len(qs), k), k, True, fam, "%s shard [%d, %d)" % (case.name, sh.r0, sh.r1))
                results.append(got)
                models.append(ms)
            end_to_end(data, data.shards, results, models, k, case.name, qs)
        for k in ks_lists:
            for sh, ix in zip(data.shards, ixs):
                ms, cap = models_of(ix, sh, data, qs, fam, k, False)
                got = scan(ix, sh, data, qs, fam, case.sim, k, answers=False)
                check(got, ms, cap, generous(ix, sh, len(qs), k), k, False, fam, "%s shard [%d, %d)" % (case.name, sh.r0, sh.r1))
                if k <= S.K_FINAL_SELECT_MAX:      # rank k: a subset of the rank k + 1 list; and the synchronous call writes the same bytes
                    with_answers = scan(ix, sh, data, qs, fam, case.sim, k)
                    plans = [[g[:5] for g in S.shard_segments(len(sh.pilot), sh.r1 - sh.r0, kd, 1024, 2)] for kd in (k, k + 1)]
                    # (where the two ranks plan the same segments: 4 k and 4 (k + 1) can round to different first segments, and then a row
                    # meets a threshold of other rows in each plan - both lists replay to the same answer, neither holds the other)
                    for q in qs if plans[0] == plans[1] else ():
                        a = got[2][got[1][q]:got[1][q + 1]]
                        b = with_answers[2][with_answers[1][q]:with_answers[1][q + 1]]
                        assert set(a.tolist()) <= set(b.tolist()), "%s: query %d's rank-k list is no subset of its rank-(k + 1) list" % (case.name, q)
                    buf = Buffers(len(qs), generous(ix, sh, len(qs), k), k, False, -1)
                    total = ix.shard_scan(data.qq, data.qc, fam.query_bits, case.sim, k, buf.packed.data_ptr(), buf.cap, buf.off.data_ptr(), buf.flags.data_ptr())
                    sync = buf.read(total)
                    for a, b in zip(sync[:3], got[:3]):
                        assert a.tobytes() == b.tobytes(), "%s: bbq_shard_scan and begin + wait without answers differ" % case.name


@pytest.mark.parametrize("case", GRID, ids=[c.name for c in GRID])
def test_grid(case):
    """every family, both row kinds, six layouts: k 1 .. 1024 with answers and end to end, 1024 / 1025 / 4096 lists only"""
    run_case(case, S.KS_ANSWERS, S.KS_LISTS)


@pytest.mark.parametrize("case", TINY, ids=[c.name for c in TINY])
def test_tiny_shards(case):
    """1 .. 513 own rows with and without a 512-row replica: rows seen below k, at k, at k + 1 and above it (take_all and its edge)"""
    run_case(case, S.TINY_KS)


@pytest.mark.parametrize("case", S.SPECIAL, ids=[c.name for c in S.SPECIAL])
def test_nan_rows_a_nan_query_and_planted_ties(case):
    run_case(case, (S.TIE_K,) if case.variant == "ties" else (10, 100), (1024,))


def test_k_beyond_the_shard_range_is_refused():
    case = GRID[1]
    data = S.case_data(case)
    sh = data.shards[1]
    with located("refused k"), opened(data, [sh], case.fam) as (ix,):
        for k, answers in S.KS_REFUSED:
            buf = Buffers(6, 1 << 16, k, answers)
            refused(lambda: buf.begin(ix, data.qq, data.qc, case.fam.query_bits, case.sim, k), capi.ERR_UNSUPPORTED, "k %d, answers %s" % (k, answers))
        refused(ix.shard_scan_wait, capi.ERR_INVALID_ARG, "wait with nothing in flight")
        ms, cap = models_of(ix, sh, data, list(range(6)), case.fam, 10, True)      # and the index serves afterwards
        check(scan(ix, sh, data, list(range(6)), case.fam, case.sim, 10), ms, cap, generous(ix, sh, 6, 10), 10, True, case.fam, "after the refusals")


# ------------------------------------------------------------------------------------------------ the floods
def _flood(which):
    data = S.flood_data("mid" if which == "mid" else "inner")
    shards = S.flood_shards(which)
    n = shards[1].r1
    return data._replace(codes=data.codes[:n], corr=data.corr[:n], scores=tuple(s[:n] for s in data.scores), n=n, shards=shards), shards


FLOOD_OPTS = {"default": {}, "flood_rows 0": {"flood_rows": 0}, "flood_rows 1024": {"flood_rows": 1024}, "sweep_share 4": {"sweep_share": 4}}


@pytest.mark.parametrize("which", ["last", "inner", "mid"])
@pytest.mark.parametrize("how", list(FLOOD_OPTS))
def test_floods(which, how):
    """rows ascending by query 0's score.  `last`: only the last own segment exceeds the key buffer - the block is unproven, cut 0, and the
    list whole: modelled completely.  `inner`: a segment that is not the last does - the cut is a subset's statistic with more than k own
    rows above it, the block is unproven and only the invariants hold.  `mid`: the same with the rows that fall off the key buffer
    mid-ranked - a PROVEN block whose cut lies below the true statistic, its entries the own rows above that cut, and the merge still
    answers like the oracle.  Every source of kFlagOverflow flags the flooding query and no other: no flood tier (flood_rows 0; the
    shared sweep of sweep_share 4), over-full chunks beyond a 1024-entry tier and the list beyond its own capacity (flood_rows 1024)"""
    data, shards = _flood(which)
    k, qs = S.FLOOD_K, list(range(len(S.FLOOD_QUERIES)))
    opts = dict(S.OPTS, **FLOOD_OPTS[how])
    with located("flood %s, %s" % (which, how)), opened(data, shards, S.W1, opts) as ixs:
        results, models = [], []
        for sh, ix in zip(shards, ixs):
            ms, cap = models_of(ix, sh, data, qs, S.W1, k, True, opts)
            got = scan(ix, sh, data, qs, S.W1, 1, k)
            check(got, ms, cap, generous(ix, sh, len(qs), k), k, True, S.W1, "flood %s shard [%d, %d)" % (which, sh.r0, sh.r1))
            results.append(got)
            models.append(ms)
        status = end_to_end(data, shards, results, models, k, "flood %s" % which, qs)
        flooding = [i for i, src in enumerate(S.FLOOD_QUERIES) if src == 0]
        if how != "default":
            assert all(status[i] == 2 for i in flooding) and all(models[1][i].flags == S.FLAG_OVERFLOW for i in flooding)
            assert results[1][0].tolist() == [S.FLAG_OVERFLOW if src == 0 else 0 for src in S.FLOOD_QUERIES]
        elif which == "mid":      # proven under a subset's cut, and merged: the oracle's answer (end_to_end has compared it)
            assert all(SUBSET[id(models[1][i])][1].ok and S.header(results[1][3][i])[3] == 0 for i in flooding)
            tied = S.merge_model([np.zeros(3, np.uint64)], data.scores[flooding[0]], k)      # (1 only where two of the k + 1 best compare equal)
            assert all(status[i] == tied for i in flooding)
        else:
            assert all(status[i] == 1 for i in flooding)      # unproven: the lists are replayed (end_to_end has compared the answer)


def test_packed_capacity():
    """generous: nothing is dropped (test_floods).  Exactly nq x bbq_shard_list_cap with three of six queries flooding: the sum does not
    fit, the squeeze round flags exactly the queries over the advertised capacity and the rest is intact.  Smaller than that and still
    not fitting: BBQ_ERR_OOM with the total reported, and the index serves the next scan"""
    data, shards = _flood("last")
    sh, k, qs = shards[1], S.FLOOD_K, list(range(len(S.FLOOD_QUERIES)))
    with located("packed capacity"), opened(data, [sh], S.W1) as (ix,):
        ms, cap = models_of(ix, sh, data, qs, S.W1, k, True)
        lengths = [len(m.rows) for m in ms]
        assert sum(lengths) > len(qs) * cap and sorted(i for i, n in enumerate(lengths) if n > cap) == [i for i, s in enumerate(S.FLOOD_QUERIES) if s == 0]
        got = scan(ix, sh, data, qs, S.W1, 1, k, cap=len(qs) * cap)
        check(got, ms, cap, len(qs) * cap, k, True, S.W1, "packed_cap = nq x list_cap")
        assert got[0].tolist() == [S.FLAG_OVERFLOW if s == 0 else 0 for s in S.FLOOD_QUERIES]
        # all six flooding: everything goes, the total is 0
        six = [0] * 6
        ms6, _ = models_of(ix, sh, data, six, S.W1, k, True)
        check(scan(ix, sh, data, six, S.W1, 1, k, cap=6 * cap), ms6, cap, 6 * cap, k, True, S.W1, "every query flooding")
        # too small for what is left behind the squeeze
        _, _, wtotal, oom = S.pack_model(lengths, [m.flags for m in ms], cap, 64)
        assert oom and wtotal > 64
        buf = Buffers(len(qs), 64, k, True)
        buf.begin(ix, data.qq, data.qc, S.W1.query_bits, 1, k)
        total = C.c_int64(-1)
        rc = capi.lib().bbq_shard_scan_wait(ix._h, C.byref(total))
        assert rc == capi.ERR_OOM and total.value == wtotal, "rc %d total %d, BBQ_ERR_OOM and %d expected" % (rc, total.value, wtotal)
        refused(ix.shard_scan_wait, capi.ERR_INVALID_ARG, "wait with nothing in flight")
        check(scan(ix, sh, data, qs, S.W1, 1, k), ms, cap, generous(ix, sh, len(qs), k), k, True, S.W1, "the scan after BBQ_ERR_OOM")


def test_a_list_of_exactly_the_advertised_capacity_survives_the_squeeze():
    """two lists of exactly bbq_shard_list_cap entries and a short one into a buffer of twice that: the squeeze round runs ("c >
    advertised_cap"), drops nothing, and the call ends in BBQ_ERR_OOM with the whole total - dropping the two would have made it fit"""
    sh, cap = S.flood_shard_at_capacity()
    data, _ = _flood("last")
    data = data._replace(codes=data.codes[:sh.r1], corr=data.corr[:sh.r1], scores=tuple(s[:sh.r1] for s in data.scores), n=sh.r1)
    qs, k = [0, 2, 1], S.FLOOD_K
    with located("a list at the advertised capacity"), opened(data, [sh], S.W1) as (ix,):
        ms, lib_cap = models_of(ix, sh, data, qs, S.W1, k, True)
        lengths = [len(m.rows) for m in ms]
        assert lib_cap == cap and lengths[:2] == [cap, cap] and not any(m.flags for m in ms)
        check(scan(ix, sh, data, qs, S.W1, 1, k), ms, cap, generous(ix, sh, 3, k), k, True, S.W1, "generous")      # the lists themselves
        wflags, _, wtotal, oom = S.pack_model(lengths, [0, 0, 0], cap, 2 * cap)
        assert oom and wtotal == sum(lengths) and not wflags.any()
        buf = Buffers(3, 2 * cap, k, True)
        buf.begin(ix, data.qq[qs], data.qc[qs], S.W1.query_bits, 1, k)
        total = C.c_int64(-1)
        rc = capi.lib().bbq_shard_scan_wait(ix._h, C.byref(total))
        assert rc == capi.ERR_OOM and total.value == wtotal, "rc %d total %d, BBQ_ERR_OOM and %d expected" % (rc, total.value, wtotal)
        assert buf.flags.cpu().numpy().tolist() == [0, 0, 0]
        got = scan(ix, sh, data, qs, S.W1, 1, k, cap=2 * cap + lengths[2])      # and with room for the sum, the same lists, nothing flagged
        check(got, ms, cap, 2 * cap + lengths[2], k, True, S.W1, "packed_cap = the sum")


# ------------------------------------------------------------------------------------------------ two in flight, the shared sweeps
@pytest.mark.parametrize("order", ["k10 first", "k1024 first"])
def test_two_batches_in_flight_with_different_k_and_nq(order):
    case = GRID[1]      # w1 ordinary, a 512-row replica
    data = S.case_data(case)
    sh, fam = data.shards[1], case.fam
    batches = [(10, [0, 1, 2, 3, 4, 5]), (1024, [4, 5])]
    if order != "k10 first":
        batches.reverse()
    with located("two in flight, %s" % order), opened(data, [sh], fam) as (ix,):
        alone = [scan(ix, sh, data, qs, fam, case.sim, k) for k, qs in batches]
        bufs = [Buffers(len(qs), generous(ix, sh, len(qs), k), k, True, -1) for k, qs in batches]
        for b, (k, qs) in zip(bufs, batches):
            b.begin(ix, data.qq[qs], data.qc[qs], fam.query_bits, case.sim, k)
        refused(lambda: Buffers(1, 1 << 14, 10, True).begin(ix, data.qq[:1], data.qc[:1], fam.query_bits, case.sim, 10), capi.ERR_INVALID_ARG, "a third batch")
        for b, (k, qs), one in zip(bufs, batches, alone):
            got = b.read(ix.shard_scan_wait())
            ms, cap = models_of(ix, sh, data, qs, fam, k, True)
            check(got, ms, cap, b.cap, k, True, fam, "in flight with another batch")
            for x, y in zip(got[:3], one[:3]):
                assert x.tobytes() == y.tobytes()
            for q, m in enumerate(ms):      # (behind a block's entries the buffer keeps what it held)
                assert got[3][q][:3 + m.n_sel].tobytes() == one[3][q][:3 + m.n_sel].tobytes()


@pytest.mark.parametrize("share", [4, 8, 32])
def test_sweep_share_changes_nothing_for_an_external_list(share):
    """an external list never sweeps on the matrix cores; sweep_share 4 / 8 sweep shared (no flood tier: the model knows), 32 per query"""
    case = GRID[1]
    data = S.case_data(case)
    sh, fam, qs = data.shards[1], case.fam, list(range(6))
    opts = dict(S.OPTS, sweep_share=share)
    with located("sweep_share %d" % share), opened(data, [sh], fam, opts) as (ix,):
        for k in (10, 100):
            ms, cap = models_of(ix, sh, data, qs, fam, k, True, opts)
            got = scan(ix, sh, data, qs, fam, case.sim, k)
            check(got, ms, cap, generous(ix, sh, 6, k), k, True, fam, "sweep_share %d" % share)
            ix.set_option("sweep_share", 1)
            one = scan(ix, sh, data, qs, fam, case.sim, k)
            ix.set_option("sweep_share", share)
            for x, y in zip(got[:3], one[:3]):
                assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ the multi-device handle
@pytest.mark.parametrize("name,n_shards,pilot_rows", [("w1-ordinary", 3, 1024), ("w1-hostile", 4, 5000), ("multibit-ordinary", 2, 0), ("nan", 3, 1024), ("ties", 2, 512)])
def test_multi_device_handle(name, n_shards, pilot_rows):
    """bbq_index_create_multi over [0] * S: the answers are the oracle's, and the statistics that bbq_multi.cpp makes functions of the
    shards' blocks are the model's: per query "status == 0: candidates += every block's m", "status 1: host_replays += 1; candidates +=
    the packed lists' lengths", "flagged: dense_fallbacks += 1; candidates += n_rows" (multi_search_batch).  The scan timings and
    resident_bytes of multi_get_stats are no functions of the scores and are left out"""
    case = {"nan": S.SPECIAL[0], "ties": S.SPECIAL[3]}.get(name) or next(c for c in GRID if c.name.startswith(name))
    data = S.case_data(case)
    fam, qs = case.fam, list(range(6))
    shards = S.multi_shards(data.n, n_shards, pilot_rows)
    with located("multi %s" % name):
        ix = B.Index.create_multi(data.codes, data.corr, fam.dim, M.CDP, [0] * n_shards, index_bits=fam.index_bits, pilot_rows=pilot_rows)
        try:
            assert ix.shards == len(shards)
            for opt, value in S.OPTS.items():
                ix.set_option(opt, value)
            for k in (S.TIE_K, 1024):
                ix.reset_stats()
                idx, sc, cnt = ix.search_batch(data.qq, data.qc, fam.query_bits, case.sim, k)
                st = ix.stats()
                want = {"candidates": 0, "host_replays": 0, "dense_fallbacks": 0}
                for q in qs:
                    oi, osc = O.heap_topk(data.scores[q], k)
                    assert cnt[q] == len(oi) and (idx[q, :cnt[q]] == oi).all() and (bits32(sc[q, :cnt[q]]) != bits32(osc)).sum() == 0, "query %d, k %d" % (q, k)
                    ms = [S.scan_model(*S.shard_scores(data, sh, q), sh.r0, k, True, S.OPTS,
                                       S.planned_list_cap(S.shard_segments(len(sh.pilot), sh.r1 - sh.r0, k + 1, 1024, 2), k + 1), fam) for sh in shards]
                    assert all(m.exact for m in ms)
                    status = S.merge_model([m.block for m in ms], data.scores[q], k)
                    if status == 0:
                        want["candidates"] += sum(m.n_sel for m in ms)
                    elif status == 1:
                        want["host_replays"] += 1
                        want["candidates"] += sum(len(m.rows) for m in ms)
                    else:
                        want["dense_fallbacks"] += 1
                        want["candidates"] += data.n
                assert {f: st[f] for f in want} == want, "k %d: the handle's statistics %s, the model's %s" % (k, {f: st[f] for f in want}, want)
        finally:
            ix.close()
