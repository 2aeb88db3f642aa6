'use strict';
// GPU: removeVectors / compactVectors of the JavaScript host against what the ctypes binding gave for the index over the kept rows
// (argv[2]: the JSON tests/test_js_compact.py wrote; argv[3]: a directory for index files).  With BBQ_DEVICES set (a multi-device
// index) the calls must throw the library's unsupported message instead.
const fs = require('fs');
const path = require('path');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const want = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dir = process.argv[3];
const sharded = !!process.env.BBQ_DEVICES;

function sameAnswer(res, w) {
  const wi = T.dec(w.idx_i32, Int32Array), ws = T.dec(w.score_f32, Float32Array);
  let ok = res.length === wi.length;
  for (let i = 0; ok && i < res.length; i++) ok = res[i].index === wi[i] && (res[i].score === ws[i] || (res[i].score !== res[i].score && ws[i] !== ws[i]));
  return ok;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }

want.cases.forEach(function (c) {
  const g = T.loadGolden(c.name), io = T.inputs(g);
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
  const mask = T.dec(c.mask_u8, Uint8Array), kept = T.dec(c.kept_i32, Int32Array);
  const codes = T.dec(c.codes_u8, Uint8Array), corr = T.dec(c.corr_f64, Float64Array), m = kept.length, rb = codes.length / m;

  // everything the compacted set answers, against the ctypes index over the kept rows
  function sameSet(index, label, searches) {
    T.check(index.size() === m, label + ': size() ' + index.size() + ' / ' + m);
    [0, 1, 63, 64, m - 2, m - 1].forEach(function (ord) {
      if (ord < 0 || ord >= m) return;
      T.check(T.sameBits(index.vectorValue(ord), codes.subarray(ord * rb, (ord + 1) * rb)), label + ': vectorValue(' + ord + ')');
      const t = index.getCorrectiveTerms(ord);
      T.check(T.sameBits(Float64Array.of(t.lowerInterval, t.upperInterval, t.additionalCorrection, t.quantizedComponentSum), corr.subarray(4 * ord, 4 * ord + 4)),
        label + ': getCorrectiveTerms(' + ord + ')');
    });
    T.check(thrown(function () { index.vectorValue(m); }) !== null, label + ': no ord behind the kept rows');
    (searches || c.answers).forEach(function (w) {
      T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[w.q], index, w.k), w), label + ' q' + w.q + ' k=' + w.k + ': top-k');
    });
  }
  function removeAndCompact(index, filterOf) {
    T.check(fmt.removeVectors(index, c.drop) === index, c.name + ': removeVectors returns targetVectors');
    T.check(index.size() === c.after_drop, c.name + ': size() after removeVectors ' + index.size());
    T.check(fmt.compactVectors(index, filterOf(index)) === index, c.name + ': compactVectors returns targetVectors');
  }

  const index = fmt.quantizeVectors(io.base).quantizedVectors;
  if (sharded) {
    fmt.searchNearestNeighbors(io.queries[0], index, 1);   // the sharded device copy is made on first search
    const msg = thrown(function () { fmt.removeVectors(index, c.drop); });
    T.check(msg !== null && /not supported on a multi-device index/.test(msg), c.name + ': a multi-device index refuses a compaction (' + msg + ')');
    T.check(index.size() === g.n && index.vectorValue(g.n - 1).length === rb, c.name + ': the refused compaction changed nothing');
    index.dispose();
    return;
  }
  // 1. host copies present, a device copy present: both are compacted
  index.vectorValue(0);
  removeAndCompact(index, function () { return mask; });
  sameSet(index, c.name + ' copies present');
  const batch = fmt.searchNearestNeighborsBatch(io.queries, index, 10);
  c.answers.filter(function (w) { return w.k === 10; }).forEach(function (w) { T.check(sameAnswer(batch[w.q], w), c.name + ' q' + w.q + ': batch'); });
  // everything kept: nothing changes; a bad ord: nothing changes
  T.check(fmt.compactVectors(index, function () { return true; }) === index && index.size() === m, c.name + ': keep all');
  T.check(thrown(function () { fmt.removeVectors(index, [m]); }) === '向量索引 ' + m + ' 不存在' && index.size() === m, c.name + ': an ord outside the set');
  T.check(thrown(function () { fmt.compactVectors(null, mask); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.compactVectors(index, new Uint8Array(m + 1)); }) !== null && index.size() === m, c.name + ': a mask of another length');
  // the filter used no longer fits, a new one does
  if (g.ib === 1) {
    const again = fmt.quantizeVectors(io.base).quantizedVectors;
    fmt.removeVectors(again, c.drop);
    const used = bbq.createRowFilter(again, mask);
    fmt.compactVectors(again, used);   // the accept set is on the device alone: the host copies are fetched again
    sameSet(again, c.name + ' by a RowFilter', c.answers.slice(0, 2));
    T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(io.queries[0], again, used, 5); }) !== null, c.name + ': the used filter is refused');
    const fresh = bbq.createRowFilter(again, function () { return true; });
    T.check(sameAnswer(fmt.searchNearestNeighborsFiltered(io.queries[c.answers[1].q], again, fresh, c.answers[1].k), c.answers[1]), c.name + ': a new filter over the compacted index');
    used.dispose(); fresh.dispose(); again.dispose();
  }
  // 2. after loadIndex the host copies are absent: they are fetched after the compaction, never before it
  const prefix = path.join(dir, c.name);
  const whole = fmt.quantizeVectors(io.base).quantizedVectors;
  fmt.saveIndex(whole, prefix);
  const loaded = fmt.loadIndex(prefix);
  removeAndCompact(loaded, function () { return Array.from(kept_after_drop(mask)); });
  sameSet(loaded, c.name + ' loaded', c.answers.slice(0, 3));
  loaded.dispose();
  // 3. without a device copy the host rows are compacted alone; the device copy made afterwards is made from them
  whole.dispose();
  removeAndCompact(whole, function () { return function (ord) { return mask[ord] !== 0; }; });
  sameSet(whole, c.name + ' host only', c.answers.slice(0, 3));
  whole.dispose();
  // the fp32 side of the rerank recipe follows
  if (g.ib === 1 && g.sim === 'COSINE') {
    const full = fmt.quantizeVectors(io.base).quantizedVectors, dv = bbq.createDeviceVectors(io.base);
    const keepAll = new Uint8Array(g.n).fill(1);
    c.drop.forEach(function (o) { keepAll[o] = 0; });
    const f1 = bbq.createRowFilter(full, keepAll);
    fmt.compactVectors(full, f1); dv.compact(f1); f1.dispose();
    const f2 = bbq.createRowFilter(full, mask);
    T.check(dv.compact(f2) === dv && dv.length === m, c.name + ': DeviceVectors.compact');
    fmt.compactVectors(full, f2); f2.dispose();
    const twin = bbq.createDeviceVectors(Array.from(kept).map(function (r) { return io.base[r]; }));
    const x = bbq.getOversampledTopKWithHeap(io.queries[0], full, dv, 10, 3, fmt), y = bbq.getOversampledTopKWithHeap(io.queries[0], index, twin, 10, 3, fmt);
    T.check(JSON.stringify(x) === JSON.stringify(y) && x.length === 10, c.name + ': rerank over compacted vectors');
    T.check(T.sameBits(dv.trueScores(io.queries[0], [0, 1, m - 1]), twin.trueScores(io.queries[0], [0, 1, m - 1])), c.name + ': true scores of kept rows');
    dv.dispose(); twin.dispose(); full.dispose();
  }
  index.dispose();
});
function kept_after_drop(mask) { const out = []; for (let i = 0; i < mask.length; i++) if (mask[i]) out.push(i); return out; }
T.finish('gpu_compact' + (sharded ? ' (sharded)' : ''));
