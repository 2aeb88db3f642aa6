"""What one ROW SHARD must leave behind a scan - its flags, its packed list, and with answers requested its answer block - as a function of
the oracle's f32 scores of the rows it has seen (its own and its pilot replica's) and the segment plan; what bbq_merge_answers must say about
the shards' blocks; and the recipe of rows, layouts and k the shard path is held to.  Numpy and the CPU oracle; nothing here touches a
device.  tests/test_shard_model_cpu.py holds the model to brute force and the recipe to its conditions; tests/test_gpu_shard_model.py
compares every word bbq_shard_scan_begin / _wait / bbq_shard_scan write with it, with no tolerance.

Everything is in KEY space (candidate_model.keys_of).  Definitions, which DESIGN.md "Row shards" repeats:

  * the LIST of a query on a shard is the set of (global row, f32 bits) of every OWN row whose key is above the threshold that stood when
    its segment ran; the threshold behind a segment is the k_dev-th largest key of all rows seen so far - pilot replica and own - and 0
    while fewer were seen.  k_dev = k + 1 with answers requested, k without (bbq_shard.cpp: "c.k_dev = answers ? k + 1 : k").  Packed,
    the list is ascending by global row (include/bbq.h, bbq_replay: "entries ascending by row");
  * the CUT is the (k + 1)-th largest key of all rows seen, 0 when at most k were seen (take_all, bbq_kernels.hip:
    "take_all = shard ? (m_new + tcount < (uint32_t)(k2 + 1))": tcount is min(rows seen before the last segment, k + 1) and with fewer
    than k + 1 seen before it the threshold is 0, so m_new is every row of the last segment);
  * the BLOCK is {entries listed | flags << 32}, {m | unproven << 32}, the cut, and the m own rows above the cut descending by key - two
    rows of one key: the larger row first, which is where the kernel's counting sort over (key << 32 | row) places them.

Rules the model takes from the source:
  * the plan (shard_segments): build_plan / add_storage_segments, bbq_core.cpp - "add_storage_segments(ix, p, 0, ix->pilot, 0, false, false,
    dummy); add_storage_segments(ix, p, 1, ix->main, ix->pilot.view.n_rows, true, true, expected_emit)", the boundary
    "nb = (before * p.growth - rows_before) / kChunkRows * kChunkRows; if (before > 0 && nb > b && nb <= R / 2) e = nb";
  * kFlagNaN: the sweeps know nothing of `emit` ("if (valid && (s32 != s32)) nan_seen = true; ... atomicOr(a.flags + q, kFlagNaN)",
    bbq_scan_body.h; the flag word is the query's, shared by every segment), so a NaN score of a PILOT row flags the query like one of an
    own row;
  * kFlagOverflow has three sources.  (1) a chunk of a sparse segment - the pilot's too - with more passing rows than cap_for(k_dev, rows
    seen before the segment) ("if (cnt > (uint32_t)a.cap)", sweep_chunk_end): with the flood tier the whole chunk moves to the query's
    overflow area while "(uint64_t)off + cnt <= (uint64_t)a.ovf_cap", off an atomic running sum over the scan, so the flag is raised iff
    the over-full chunks of the whole scan hold more than flood_cap entries together; the shared sweep of sweep_share 4 / 8 has no such
    tier ("if (cnt > (uint32_t)a.cap) ... atomicOr(a.flags + q0 + b, kFlagOverflow)", bbq_kernels.hip) and sweep_share 32 does not
    reach an external list ("use_mfma = !ext && ...", enqueue_subbatch), it sweeps per query.  (2) the list itself: "if (base + m_new >
    a.list_cap) flags |= kFlagOverflow" with the scan's own capacity "plan.list_cap + std::min<int64_t>(plan.flood_cap, 65536)"
    (bbq_shard.cpp).  (3) the pack kernel's squeeze round (pack_model): "if (!f && squeeze && (int64_t)c > advertised_cap)", entered only
    when the first round's sum exceeds packed_cap;
  * the `ok` chain of the last finalize launch: no flag, "total <= a.list_cap", "m_new <= (uint32_t)kFinalizeKeyCap - tcount", and behind
    the selection "n_sel <= (uint32_t)k2" - which an order statistic of rank k + 1 over ALL rows seen never fails (one over a subset can: see
    `exact`).  Not ok: {0 | unproven}, cut 0, no entry.

`exact` is False where a segment that is NOT the last brought more new keys than the finalize kernel's LDS holds beside the running top
keys ("m_use = min(m_new, kFinalizeKeyCap - tcount)"): every later threshold and the cut are then order statistics of whichever subset
fitted.  The model then returns the lists and the cut of the TRUE statistics, and what holds of the device's is: its list is a superset,
its cut is at most the true cut, and proven entries are exactly the own rows above ITS cut.  scan_model(subset=True) follows the keys that
fit instead - in list order, the first kFinalizeKeyCap - tcount of the segment - and says whether such a block is proven: in the `inner`
flood 21 own rows lie above the subset's cut and "n_sel <= k2" leaves it unproven, in the `mid` flood 5 do and the block is proven with
a cut two ranks below the true one.

Left out: the `entries listed` half of slot 0 of a FLAGGED query.  A flagged query carries no list (its offsets are equal), and what the
launch counted before it was flagged depends on where a NaN's bit pattern sorts and on which chunks were truncated."""
import collections
import functools

import numpy as np

import call_walk as W
import candidate_model as M
import orclib as O
from candidate_model import FAMILIES, PLAN, keys_of, kth_largest, queries, rows, scores, scores_of_keys  # noqa: F401  (the model's vocabulary)
from call_walk import K_FINAL_SELECT_MAX, K_MAX_FAST_K, plan_segments  # noqa: F401

F32 = np.float32
CHUNK = 512
KEY_CAP = M.K_FINALIZE_KEY_CAP
FLAG_OVERFLOW, FLAG_NAN = 1, 2      # kFlagOverflow, kFlagNaN (bbq_device.h)
U32 = np.uint64(0xFFFFFFFF)


def shard_block(s32, keys, r0, r1, pilot, k, stride):
    """the block of the shard [r0, r1) with a pilot replica of the global prefix [0, pilot), by the definition alone (no plan, no
    capacities): what the last finalize launch leaves when nothing overflows.  Equal keys: the larger row first"""
    blk = np.zeros(stride, np.uint64)
    seen = np.unique(np.concatenate([np.arange(0, pilot if r0 > 0 else 0), np.arange(r0, r1)])).astype(np.int64)
    ks = np.sort(keys[seen])[::-1]
    cut = int(ks[k]) if len(ks) >= k + 1 else 0
    own = np.arange(r0, r1)
    own = own[keys[own] > cut][::-1]
    own = own[np.argsort(-keys[own].astype(np.int64), kind="stable")]
    assert len(own) <= k
    blk[1], blk[2] = len(own), cut
    blk[3:3 + len(own)] = (own.astype(np.uint64) << np.uint64(32)) | s32[own].view(np.uint32).astype(np.uint64)
    return blk


# ------------------------------------------------------------------------------------------------ the plan

Segment = collections.namedtuple("Segment", "storage first rows dense emit before")      # storage 0: the pilot replica, 1: the own rows


def cap_for(k_dev, rows_before):
    """cap_for, bbq_core.cpp: candidate slots per chunk of a sparse segment"""
    lam = k_dev * CHUNK / max(rows_before, 1)
    c = int(np.ceil(lam + 8.0 * np.sqrt(lam) + 16.0))
    c = (c + 7) // 8 * 8
    return min(max(c, 16), CHUNK)


def shard_segments(pilot_rows, own_rows, k_dev, first_segment_rows, growth):
    """build_plan / add_storage_segments (bbq_core.cpp): the pilot replica's storage first - dense, then sparse, nothing emitted -, then the
    shard's own with rows_before = pilot_rows and have_theta: sparse from its first row.  Without a replica the own storage starts dense"""
    s0 = min(max(first_segment_rows, (4 * k_dev + CHUNK - 1) // CHUNK * CHUNK), 8192)      # start_plan
    segs = []

    def storage(which, R, rows_before, have_theta, emit):
        if R <= 0:
            return
        b = 0
        if not have_theta:
            rows_before = 0
            b = min(s0, R)
            segs.append(Segment(which, 0, b, True, emit, 0))
        while b < R:
            before = rows_before + b
            e, nb = R, (before * growth - rows_before) // CHUNK * CHUNK
            if before > 0 and nb > b and nb <= R // 2:
                e = nb
            segs.append(Segment(which, b, e - b, False, emit, before))
            b = e

    if pilot_rows > 0:
        storage(0, pilot_rows, 0, False, False)
        storage(1, own_rows, pilot_rows, True, True)
    else:
        storage(1, own_rows, 0, False, True)
    return segs


def planned_list_cap(segs, k_dev):
    """size_plan, bbq_core.cpp: "everything listed whole + 4x the expected sparse candidates + slack".  What bbq_shard_list_cap returns for
    the plan of rank k_dev; the GPU test asserts that and hands the library's figure to scan_model, the CPU test has only this one"""
    whole = sum(g.rows for g in segs if g.emit and g.dense)
    expected = 0.0      # summed in the plan's order, as the source does
    for g in segs:
        if g.emit:
            expected += float(g.rows) if g.dense else float(k_dev) * float(g.rows) / float(g.before)
    cap = whole + int(4.0 * max(0.0, expected - float(whole))) + 4096
    return (cap + 1023) // 1024 * 1024


def flood_cap_of(own_rows, opts):
    """size_plan, bbq_core.cpp: the query's overflow area, in entries"""
    cap = min(M.option(opts, "flood_rows"), (own_rows + 1023) // 1024 * 1024)
    if cap > 0:
        batch = M.option(opts, "batch_queries") or 128      # effective_batch: an explicit value as it is; these sizes: at most 128
        cap = min(cap, max(16384, ((64 << 20) // max(32, batch)) // 1024 * 1024))
    return cap


def shared_sweep(fam, opts, cap):
    """does a sparse segment of this scan run on the shared sweep (no flood tier)?  enqueue_subbatch + shared_sweep_supported"""
    share = M.option(opts, "sweep_share")
    w16 = W.w16_of(fam.dim, fam.index_bits) if fam is not None else 0
    return share in (4, 8) and fam is not None and fam.index_bits == 1 and w16 in (1, 6, 8, 12) and share * cap * 8 < 48 * 1024


# ------------------------------------------------------------------------------------------------ one query on one shard

Scan = collections.namedtuple("Scan", "flags reasons rows bits split thetas block exact cut branch n_sel seen pilot_above take_all ok why_not own "
                              "row_base m_last tcount room")


def scan_model(pilot_scores, own_scores, row_base, k, answers, opts, list_cap, fam=None, subset=False):
    """ONE query on ONE shard.  pilot_scores / own_scores: the oracle's f32 scores of the replica's rows and of the shard's own;
    answers: is dev_answers passed; list_cap: the advertised capacity (bbq_shard_list_cap), an input.  Returns Scan:
      flags, reasons     what the finalize launches leave in the query's flag word (the squeeze is the batch's: pack_model), and why
      rows, bits         the list: global rows ascending, their f32 bits; split / thetas: entries per own segment, the threshold every
                         segment of the plan ran against (0 for a dense one)
      block              with answers: uint64 [3 + m], slot 0's `listed` half included for an unflagged query
      exact              see the module's docstring; cut / branch / n_sel / seen / pilot_above / take_all / ok / why_not / m_last / tcount /
                         room: the last launch's figures
    subset: where a segment that is not the last brings more new keys than fit, go on with the keys that DO fit instead of the true
    statistic - in the chunk-slot mode every shard scan runs in, the first kFinalizeKeyCap - tcount entries of the segment in list order
    ("if (j < (uint32_t)kFinalizeKeyCap) s_keys[j] = ...", then the running keys land behind m_use).  Scan.exact is False either way; the
    subset scan is what the recipe's reach conditions and the expected `unproven` of an inexact block are read from."""
    ps, ow = np.ascontiguousarray(pilot_scores, F32), np.ascontiguousarray(own_scores, F32)
    k_dev = k + 1 if answers else k
    segs = shard_segments(len(ps), len(ow), k_dev, M.option(opts, "first_segment_rows"), M.option(opts, "segment_growth"))
    flood_cap = flood_cap_of(len(ow), opts)
    room = list_cap + min(flood_cap, 65536)
    flags, reasons = 0, []
    if np.isnan(ps).any():
        flags |= FLAG_NAN
        reasons.append("a NaN score in the pilot replica")
    if np.isnan(ow).any():
        flags |= FLAG_NAN
        reasons.append("a NaN score in the own rows")
    pk, okeys = keys_of(ps), keys_of(ow)
    theta, exact, n_seen = 0, True, 0
    run = np.zeros(0, np.uint32)      # the running top keys: the k_dev largest of the keys taken in so far (all of them while fewer)
    listed, split, thetas, parked, base, m_last, last_keys = [], [], [], 0, 0, 0, run
    for i, g in enumerate(segs):
        src = pk if g.storage == 0 else okeys
        here = src[g.first:g.first + g.rows]
        passing = np.ones(len(here), bool) if g.dense else here > theta
        thetas.append(0 if g.dense else theta)
        m_new = int(passing.sum())
        if not g.dense:
            cap = cap_for(k_dev, g.before)
            per_chunk = np.add.reduceat(passing.astype(np.int64), np.arange(0, len(here), CHUNK))
            over = per_chunk[per_chunk > cap]
            if len(over) and (shared_sweep(fam, opts, cap) or flood_cap == 0):
                flags |= FLAG_OVERFLOW
                reasons.append("segment %d: a chunk with %d passing rows over %d slots, no flood tier" % (i, over.max(), cap))
            parked += int(over.sum())
        if g.emit:
            at = np.flatnonzero(passing) + g.first
            listed.append(at)
            split.append(m_new)
            base += m_new
            if base > room:
                flags |= FLAG_OVERFLOW
                reasons.append("segment %d: %d entries over the list's %d" % (i, base, room))
        n_seen += len(here)
        new = here[passing]      # (a row at or below the threshold is not among the k_dev largest: leaving it out changes no statistic)
        if i + 1 == len(segs):      # (size_plan: "p.segs.back().need_theta = false")
            m_last, last_keys = m_new, new
            break
        if m_new > KEY_CAP - len(run):
            exact = False
            if subset:
                new = new[:KEY_CAP - len(run)]
        run = np.sort(np.concatenate([run, new]))[::-1][:k_dev]
        theta = int(run[k_dev - 1]) if len(run) >= k_dev else 0
    tcount = len(run)
    if parked > flood_cap > 0:
        flags |= FLAG_OVERFLOW
        reasons.append("%d entries of over-full chunks over the flood tier's %d" % (parked, flood_cap))
    at = np.concatenate(listed) if listed else np.zeros(0, np.int64)
    lrows, lbits = at + row_base, ow[at].view(np.uint32)
    block, cut, branch, n_sel, take_all, ok, why_not, pilot_above = None, 0, None, 0, False, False, None, 0
    if answers:
        k2 = k
        total = base
        take_all = m_last + tcount < k2 + 1
        why_not = ("flags" if flags else "total > list_cap" if total > room else
                   "m_new > kFinalizeKeyCap - tcount" if m_last > KEY_CAP - tcount else
                   "the last launch emits nothing" if segs and not segs[-1].emit else None)      # ("... && a.emit && ...": a replica and no own row)
        ok = why_not is None and len(segs) > 0
        block = [np.uint64(min(total, room)) | (np.uint64(flags) << np.uint64(32)), np.uint64(1) << np.uint64(32), np.uint64(0)]
        if ok:
            if take_all:
                sel = np.arange(len(at))
                branch = "take_all"
            else:
                cut = kth_largest(np.concatenate([run, last_keys]), k2 + 1)
                branch = "count" if m_last + tcount <= 2048 else "radix"
                sel = np.flatnonzero(okeys[at] > cut)
            n_sel = len(sel)
            assert n_sel <= k2 or not exact, "an order statistic of rank k + 1 over all rows seen has at most k rows above it"
            pilot_above = int((pk > cut).sum()) if not take_all else 0
            if n_sel > k2:      # (a subset's statistic: "ok = shard ? (n_sel <= (uint32_t)k2)")
                ok, why_not, cut = False, "n_sel > k2", 0
            else:
                order = sel[::-1]
                order = order[np.argsort(-okeys[at][order].astype(np.int64), kind="stable")]
                block[1], block[2] = np.uint64(n_sel), np.uint64(cut)
                block += list((lrows[order].astype(np.uint64) << np.uint64(32)) | lbits[order].astype(np.uint64))
        if not segs:
            block = [np.uint64(0)] * 3      # "a shard without rows ... launches nothing": all-zero blocks (enqueue_subbatch)
        block = np.array(block, np.uint64)
    return Scan(flags=flags, reasons=tuple(reasons), rows=lrows, bits=lbits, split=tuple(split), thetas=tuple(thetas), block=block, exact=exact,
                cut=cut, branch=branch, n_sel=n_sel, seen=n_seen, pilot_above=pilot_above, take_all=take_all, ok=ok, why_not=why_not, own=ow,
                row_base=row_base, m_last=m_last, tcount=tcount, room=room)


def pack_model(lengths, flags, list_cap, packed_cap):
    """bbq_pack_offsets_kernel over one batch: (flags out, offsets [nq + 1], total, does bbq_shard_scan_wait return BBQ_ERR_OOM).  A flagged
    query carries no entries; only if the sum then exceeds packed_cap the squeeze round drops (flags) every query whose list is longer
    than the advertised capacity - "(int64_t)c > advertised_cap" - and what is left fits any buffer of nq * list_cap entries"""
    lengths, flags = np.asarray(lengths, np.int64), np.asarray(flags, np.int32).copy()
    carried = np.where(flags != 0, 0, lengths)
    if carried.sum() > packed_cap:
        flags[(flags == 0) & (lengths > list_cap)] = FLAG_OVERFLOW
        carried = np.where(flags != 0, 0, lengths)
    offsets = np.concatenate([[0], np.cumsum(carried)]).astype(np.int64)
    return flags, offsets, int(offsets[-1]), bool(offsets[-1] > packed_cap)


def header(block):
    """(entries listed, flags, m, unproven, cut) of a block"""
    b = np.asarray(block, np.uint64)
    return int(b[0] & U32), int(b[0] >> np.uint64(32)), int(b[1] & U32), int(b[1] >> np.uint64(32)), int(b[2])


def merge_model(blocks, scores_q, k):
    """the status bbq_merge_answers gives ONE query from its sources' blocks and the oracle's scores of ALL rows: 2 where a source flagged
    it, 1 where a source is unproven or two of the k + 1 largest scores compare equal as floats (+0 == -0), 0 otherwise - and then the
    answer is the oracle's heap_topk.  (Above max(cut) lie at most k + 1 merged entries; fewer than k, or k with the last equal to the
    cut's score, means a tie at the edge: bbq_replay.cpp)"""
    hs = [header(b) for b in blocks]
    if any(h[1] for h in hs):
        return 2
    if any(h[3] for h in hs):
        return 1
    s = np.asarray(scores_q, F32)
    top = scores_of_keys(np.sort(keys_of(s))[::-1][:k + 1]).astype(np.float64)
    return 1 if len(np.unique(top)) != len(top) else 0


# ------------------------------------------------------------------------------------------------ the recipe

SHARD_FAMILIES = tuple(M.BY_NAME[n] for n in ("w1", "generic", "w6", "w12", "multibit"))
ROW_KINDS = M.ROW_KINDS
KS_ANSWERS = (1, 10, 100, 1023, 1024)
KS_LISTS = (1024, 1025, 4096)
KS_REFUSED = ((1025, True), (4097, False))      # (k, with answers): BBQ_ERR_UNSUPPORTED
TINY_OWN = (1, 63, 64, 65, 511, 513)
TINY_KS = (1, 10, 64, 100, 1023, 1024)          # rows seen 63 / 64 / 65 / 511 around k = 64; with the 512-row replica 1023 and 1025 around 1023, 1024
OPTS = dict(PLAN, batch_queries=2)              # slots are reused inside a batch of six queries
ALL_PILOT_BASE = 1237                           # n_pilot == row_base, no multiple of 512: the one such case bbq_index_create_shard admits

Shard = collections.namedtuple("Shard", "r0 r1 pilot")      # own rows [r0, r1); pilot: the replica's global rows in the replica's order (distinct, all < r0)
NONE = np.zeros(0, np.int64)


def half_of(fam):
    return 2048 if fam.n < 8192 else 4096


def layouts(fam):
    """{name: (rows of the family used, [Shard])}"""
    n, h = fam.n, half_of(fam)
    third = -(-n // 3 // CHUNK) * CHUNK
    quarter = n // 4 // CHUNK * CHUNK      # (rounded down: the ragged last shard is the largest)
    out = {
        "no replica": (n, [Shard(0, h, NONE), Shard(h, n, NONE)]),
        "prefix 512": (n, [Shard(0, h, NONE), Shard(h, n, np.arange(512))]),
        "whole prefix": (n, [Shard(0, ALL_PILOT_BASE, NONE), Shard(ALL_PILOT_BASE, n, np.arange(ALL_PILOT_BASE))]),
        "strided 1024": (n, [Shard(0, h, NONE), Shard(h, n, np.arange(1024) * (h // 1024) + (h // 1024 - 1))]),
        "three": (n, [Shard(0, third, NONE), Shard(third, 2 * third, np.arange(1024)), Shard(2 * third, n, np.arange(1024))]),
        "four": (n, [Shard(s * quarter, (s + 1) * quarter if s < 3 else n, np.arange(512) if s else NONE) for s in range(4)]),
    }
    for t in TINY_OWN:
        out["tiny %d" % t] = (h + t, [Shard(0, h, NONE), Shard(h, h + t, NONE)])
        out["tiny %d + 512" % t] = (h + t, [Shard(0, h, NONE), Shard(h, h + t, np.arange(512))])
    return out


GRID_LAYOUTS = ("no replica", "prefix 512", "whole prefix", "strided 1024", "three", "four")
TINY_FAMILIES = ("w1", "multibit")

Case = collections.namedtuple("Case", "name fam kind sim layout variant")


def grid_cases():
    out = []
    for fi, fam in enumerate(SHARD_FAMILIES):
        for ki, kind in enumerate(ROW_KINDS):
            for li, lay in enumerate(GRID_LAYOUTS):
                out.append(Case("%s-%s-%s" % (fam.name, kind, lay.replace(" ", "_")), fam, kind, (fi + ki + li) % 3, lay, None))
    return out


def tiny_cases():
    return [Case("%s-%s" % (name, lay.replace(" ", "_")), M.BY_NAME[name], "ordinary", 1 + i % 2, lay, None)
            for i, name in enumerate(TINY_FAMILIES) for lay in layouts(M.BY_NAME[name]) if lay.startswith("tiny")]


W1 = M.BY_NAME["w1"]
NAN_OWN_ROW, NAN_PILOT_ROW, NAN_QUERY = half_of(W1) + 700, 100, 3
TIE_K = 10
SPECIAL = (Case("nan-own-row", W1, "ordinary", 1, "prefix 512", "nan own"),
           Case("nan-pilot-row", W1, "ordinary", 1, "prefix 512", "nan pilot"),
           Case("nan-query", W1, "ordinary", 1, "prefix 512", "nan query"),
           Case("ties", W1, "ordinary", 1, "prefix 512", "ties"))

Data = collections.namedtuple("Data", "codes corr qq qc scores n shards")


@functools.lru_cache(maxsize=4)
def case_data(case):
    """the rows, queries, oracle scores (per query, over the n rows used) and shards of a case: seeded, read-only"""
    fam = case.fam
    n, shards = layouts(fam)[case.layout]
    codes, corr = rows(fam, case.kind)
    qq, qc = queries(fam, case.sim)
    if case.variant is None:
        sc = tuple(s[:n] for s in scores(fam, case.kind, case.sim))
        return Data(codes[:n], corr[:n], qq, qc, sc, n, shards)
    codes, corr, qc = codes.copy(), corr.copy(), qc.copy()
    if case.variant == "nan own":
        corr[NAN_OWN_ROW, 2] = np.nan
    elif case.variant == "nan pilot":
        corr[NAN_PILOT_ROW, 2] = np.nan
    elif case.variant == "nan query":
        qc[NAN_QUERY, 2] = np.nan
    elif case.variant == "ties":
        best = int(np.argmax(scores(fam, case.kind, case.sim)[0]))
        at = np.concatenate([np.arange(6) * 80 + 11, half_of(fam) + np.arange(TIE_K + 2 - 6) * 300 + 5])      # six in the replica's rows (the root's own), six in the shard's
        codes[at], corr[at] = codes[best], corr[best]
    sc = tuple(M.score(fam, codes, corr, qq[q], qc[q], case.sim) for q in range(len(qq)))
    for a in (codes, corr, qc) + sc:
        a.setflags(write=False)
    return Data(codes, corr, qq, qc, sc, n, shards)


def shard_scores(data, shard, q):
    """(pilot scores, own scores) of query q on a shard"""
    return data.scores[q][shard.pilot], data.scores[q][shard.r0:shard.r1]


# The floods: w1 rows, a 3072-row root and ONE shard behind it whose replica is the whole root.
#   * Rows [0, 24576) ascend by query 0's score - every one of them enters the reference heap - and the lowest-scoring 21504 rows of
#     all lie behind them, so the last own segment of the longest layout lists next to nothing and its finalize launch goes all the
#     way to the n_sel test.
#   * The replica is handed over in DESCENDING row order.  Ascending, its own sparse segments flood too and their over-full chunks
#     take 2048 entries of the query's overflow area (one area per query and scan, sized by the own rows): the model flags the query.
#   * The own segments end at own rows 3072, 9216 and 21504 (the rows seen double: 6144, 12288, 24576).
#   * `last` is the smallest shard whose LAST own segment exceeds 12288 - (k + 1) entries for query 0 while no earlier one does.
#   * `inner` is the smallest with a boundary at 21504 (21504 <= R / 2): its segment [9216, 21504) is not the last and brings 12288 rows.
#     The keys that fit are the first 12277 in list order, so the 11 that fall off are the best of the segment: 21 own rows lie above
#     the subset's cut and the launch leaves the block unproven.
#   * `mid` is `inner` over rows moved so that the subset's cut PROVES a block (flood_data).
FLOOD_K = 10
FLOOD_BASE = 3072
FLOOD_OWN = {"last": 9216 + KEY_CAP - (FLOOD_K + 1) + 1, "inner": 2 * 21504, "mid": 2 * 21504}
FLOOD_ASCENDING = FLOOD_BASE + 21504      # global rows [0, this) ascend
FLOOD_QUERIES = (0, 1, 0, 2, 0, 3)      # the flooding query three times among three that do not flood
MID_REPLICA_RANKS = 7                   # `mid`: the best 7 rows go to the replica ...
MID_TAIL_RANKS = (22, 21, 20, 19, 18, 17, 16, 13, 12, 9, 8, 15, 14, 11, 10)      # ... and ranks 22 .. 8 end the inner segment so


@functools.lru_cache(maxsize=2)
def flood_data(which="inner"):
    """Data of the largest flood layout; `last` is a prefix of its rows.  `mid`: the same rows with the ascending part's best 7 swapped
    into the replica (for the 7 lowest rows of all, which are listed nowhere) and its ranks 22 .. 8 reordered to MID_TAIL_RANKS: of the
    inner segment's 12281 listed entries the last 4 fall off the key buffer - ranks 15, 14, 11, 10 - so the running keys are ranks
    1 .. 9, 12, 13, the device's cut is rank 13 where the true one is rank 11, and 5 own rows (ranks 8 .. 12) lie above it: proven"""
    n = FLOOD_BASE + max(FLOOD_OWN.values())
    codes, corr = M.ordinary_rows(W1, n, salt=3)
    qq, qc = queries(W1, 1)
    s0 = M.score(W1, codes, corr, qq[0], qc[0], 1)
    order = np.argsort(s0, kind="stable")
    tail = n - FLOOD_ASCENDING
    order = np.concatenate([order[tail:], order[:tail]])
    if which == "mid":
        top = FLOOD_ASCENDING      # the row of rank r of the ascending part sits at top - r
        moved = order.copy()
        for r in range(1, MID_REPLICA_RANKS + 1):
            moved[r - 1], moved[top - r] = order[top - r], order[r - 1]
        first = top - MID_TAIL_RANKS[0]
        for j, r in enumerate(MID_TAIL_RANKS):
            moved[first + j] = order[top - r]
        assert sorted(moved.tolist()) == sorted(order.tolist())
        order = moved
    codes, corr = codes[order].copy(), corr[order].copy()
    distinct = {q: M.score(W1, codes, corr, qq[q], qc[q], 1) for q in sorted(set(FLOOD_QUERIES))}
    sc = tuple(distinct[q] for q in FLOOD_QUERIES)
    qq, qc = qq[list(FLOOD_QUERIES)], qc[list(FLOOD_QUERIES)]
    for a in (codes, corr) + sc:
        a.setflags(write=False)
    return Data(codes, corr, qq, qc, sc, n, None)


def flood_shards(which):
    return [Shard(0, FLOOD_BASE, NONE), Shard(FLOOD_BASE, FLOOD_BASE + FLOOD_OWN[which], np.arange(FLOOD_BASE)[::-1].copy())]


def flood_shard_at_capacity(k=FLOOD_K, opts=None):
    """(Shard, advertised capacity) behind the flood's root whose list for query 0 holds EXACTLY the advertised capacity - the edge of the
    squeeze round's "c > advertised_cap": such a list stays.  One own segment (the boundary 3072 is beyond half its rows), every own row
    above the replica's threshold listed; the own rows that tie with that threshold are not, so the size is searched from the model"""
    data, opts = flood_data(), opts or OPTS
    for own in range(5120, 5120 + 256):
        sh = Shard(FLOOD_BASE, FLOOD_BASE + own, np.arange(FLOOD_BASE)[::-1].copy())
        segs = shard_segments(FLOOD_BASE, own, k + 1, opts["first_segment_rows"], opts["segment_growth"])
        cap = planned_list_cap(segs, k + 1)
        m = scan_model(data.scores[0][sh.pilot], data.scores[0][sh.r0:sh.r1], sh.r0, k, True, opts, cap, W1)
        if len(m.rows) == cap and not m.flags:
            return sh, cap
    raise AssertionError("no flood shard whose list is exactly the advertised capacity")


def multi_shards(n, n_shards, pilot_rows):
    """the shards bbq_index_create_multi_opts makes (bbq_multi.cpp): "per = max(kChunkRows, ((n_rows + n_shards - 1) / n_shards + kChunkRows -
    1) / kChunkRows * kChunkRows)", the last takes the remainder, empty ones are not created, and "if (r0 > 0) P = pilot_rows >= r0 ? r0 :
    pilot_rows / kChunkRows * kChunkRows\""""
    per = max(CHUNK, ((n + n_shards - 1) // n_shards + CHUNK - 1) // CHUNK * CHUNK)
    out = []
    for s in range(n_shards):
        r0 = min(s * per, n)
        r1 = n if s == n_shards - 1 else min(r0 + per, n)
        if r1 <= r0 and s != 0:
            continue
        P = 0 if r0 == 0 else (r0 if pilot_rows >= r0 else pilot_rows // CHUNK * CHUNK)
        out.append(Shard(r0, r1, np.arange(P)))
    return out
