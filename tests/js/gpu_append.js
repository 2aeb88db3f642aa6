'use strict';
// GPU: appendVectors of the JavaScript host against what the ctypes binding gave for the same rows (argv[2]: the JSON
// tests/test_js_append.py wrote; argv[3]: a directory for index files).  With BBQ_DEVICES set (a multi-device index) the call must throw
// the library's unsupported message instead.
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
function sameRows(index, c, g, label) {
  const codes = T.dec(c.new_codes_u8, Uint8Array), corr = T.dec(c.new_corr_f64, Float64Array);
  const rb = codes.length / (g.n - c.cut);
  [c.cut, c.cut + 1, g.n - 1].forEach(function (ord) {
    const j = ord - c.cut;
    T.check(T.sameBits(index.vectorValue(ord), codes.subarray(j * rb, (j + 1) * rb)), label + ': vectorValue(' + ord + ')');
    const t = index.getCorrectiveTerms(ord);
    T.check(T.sameBits(Float64Array.of(t.lowerInterval, t.upperInterval, t.additionalCorrection, t.quantizedComponentSum), corr.subarray(4 * j, 4 * j + 4)),
      label + ': getCorrectiveTerms(' + ord + ')');
  });
  T.check(thrown(function () { index.vectorValue(g.n); }) !== null, label + ': no ord behind the new rows');
}

want.cases.forEach(function (c) {
  const g = T.loadGolden(c.name), io = T.inputs(g);
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
  const a = io.base.slice(0, c.cut), b = io.base.slice(c.cut);
  const index = fmt.quantizeVectors(a).quantizedVectors;
  if (sharded) {
    const msg = thrown(function () { fmt.appendVectors(index, b); });
    T.check(msg !== null && /not supported on a multi-device index/.test(msg), c.name + ': a multi-device index refuses an append (' + msg + ')');
    T.check(index.size() === c.cut, c.name + ': the refused append changed nothing');
    index.dispose();
    return;
  }
  const first = Uint8Array.from(index.vectorValue(0));
  const cap = index.reserve(g.n);
  T.check(cap >= g.n && cap % 64 === 0, c.name + ': reserve gives whole tiles (' + cap + ')');
  const mid = c.cut + Math.floor(b.length / 2);
  T.check(fmt.appendVectors(index, io.base.slice(c.cut, mid)) === index, c.name + ': appendVectors returns targetVectors');
  fmt.appendVectors(index, io.base.slice(mid));
  T.check(index.reserve(0) === cap, c.name + ': appends inside the reservation keep the capacity');
  T.check(index.size() === c.size && c.size === g.n, c.name + ': size() ' + index.size());
  T.check(T.sameBits(index.vectorValue(0), first), c.name + ': old rows unchanged');
  sameRows(index, c, g, c.name);
  c.answers.forEach(function (w) {
    T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[w.q], index, w.k), w), c.name + ' q' + w.q + ' k=' + w.k + ': top-k after appendVectors');
  });
  const ks = Array.from(new Set(c.answers.map(function (w) { return w.k; })));
  ks.forEach(function (k) {
    const batch = fmt.searchNearestNeighborsBatch(io.queries, index, k);
    c.answers.filter(function (w) { return w.k === k; }).forEach(function (w) { T.check(sameAnswer(batch[w.q], w), c.name + ' q' + w.q + ' k=' + k + ': batch'); });
  });
  // validation: nothing changes on an error
  T.check(thrown(function () { fmt.appendVectors(null, b); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.appendVectors(index, [new Float32Array(g.dim + 1)]); }) !== null, 'dimension');
  const bad = [Float32Array.from(b[0])]; bad[0][0] = NaN;
  const msg = thrown(function () { fmt.appendVectors(index, bad); });
  T.check(msg !== null && /向量 0 位置 0 包含NaN值/.test(msg), c.name + ': NaN is refused with its position (' + msg + ')');
  T.check(fmt.appendVectors(index, []) === index && index.size() === g.n, c.name + ': an empty block');
  // a filter made before an append no longer fits; a new one does
  if (g.ib === 1) {
    const small = fmt.quantizeVectors(a).quantizedVectors, old = bbq.createRowFilter(small, function () { return true; });
    fmt.appendVectors(small, b);
    T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(io.queries[0], small, old, 5); }) !== null, c.name + ': the old filter is refused');
    const fresh = bbq.createRowFilter(small, function () { return true; });
    T.check(sameAnswer(fmt.searchNearestNeighborsFiltered(io.queries[c.answers[1].q], small, fresh, c.answers[1].k), c.answers[1]), c.name + ': a new filter over the grown index');
    old.dispose(); fresh.dispose(); small.dispose();
  }
  // a loaded index fetches its host copies lazily: after an append they cover the new rows
  const prefix = path.join(dir, c.name);
  const part = fmt.quantizeVectors(a).quantizedVectors;
  fmt.saveIndex(part, prefix);
  part.dispose();
  const loaded = fmt.loadIndex(prefix);
  fmt.appendVectors(loaded, b);
  T.check(loaded.size() === g.n, c.name + ': loaded + appended size()');
  sameRows(loaded, c, g, c.name + ' loaded');
  T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[c.answers[0].q], loaded, c.answers[0].k), c.answers[0]), c.name + ': loaded + appended top-k');
  loaded.dispose();
  // the fp32 side of the rerank recipe grows with the index
  if (g.ib === 1 && g.sim === 'COSINE') {
    const dv = bbq.createDeviceVectors(a), whole = bbq.createDeviceVectors(io.base);
    T.check(dv.append(b) === dv && dv.length === g.n, c.name + ': DeviceVectors.append');
    const x = bbq.getOversampledTopKWithHeap(io.queries[0], index, dv, 10, 3, fmt), y = bbq.getOversampledTopKWithHeap(io.queries[0], index, whole, 10, 3, fmt);
    T.check(JSON.stringify(x) === JSON.stringify(y) && x.length === 10, c.name + ': rerank over appended vectors');
    T.check(T.sameBits(dv.trueScores(io.queries[0], [0, c.cut, g.n - 1]), whole.trueScores(io.queries[0], [0, c.cut, g.n - 1])), c.name + ': true scores of new rows');
    dv.dispose(); whole.dispose();
  }
  index.dispose();
});
T.finish('gpu_append' + (sharded ? ' (sharded)' : ''));
