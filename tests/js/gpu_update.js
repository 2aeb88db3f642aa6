'use strict';
// GPU: updateVectors of the JavaScript host against what the ctypes binding gave for the same rows (argv[2]: the JSON
// tests/test_js_update.py wrote; argv[3]: a directory for index files).  With BBQ_DEVICES set (a multi-device index) the call must throw
// the library's unsupported message instead; with BBQ_HOST_QUANTIZER=1 the rows are quantized on the host and the results are the same.
const fs = require('fs');
const path = require('path');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const want = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dir = process.argv[3];
const sharded = !!process.env.BBQ_DEVICES, hostQuantizer = process.env.BBQ_HOST_QUANTIZER === '1';

function sameAnswer(res, w) {
  const wi = T.dec(w.idx_i32, Int32Array), ws = T.dec(w.score_f32, Float32Array);
  let ok = res.length === wi.length;
  for (let i = 0; ok && i < res.length; i++) ok = res[i].index === wi[i] && (res[i].score === ws[i] || (res[i].score !== res[i].score && ws[i] !== ws[i]));
  return ok;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }
// the rows at the updated ords are the block's - of equal ords the last - and a row that was not named is the untouched one
function sameRows(index, c, untouched, label) {
  const codes = T.dec(c.block_codes_u8, Uint8Array), corr = T.dec(c.block_corr_f64, Float64Array);
  const rb = codes.length / c.ords.length, last = {};
  c.ords.forEach(function (o, i) { last[o] = i; });
  Object.keys(last).forEach(function (o) {
    const j = last[o], ord = Number(o);
    T.check(T.sameBits(index.vectorValue(ord), codes.subarray(j * rb, (j + 1) * rb)), label + ': vectorValue(' + ord + ')');
    const t = index.getCorrectiveTerms(ord);
    T.check(T.sameBits(Float64Array.of(t.lowerInterval, t.upperInterval, t.additionalCorrection, t.quantizedComponentSum), corr.subarray(4 * j, 4 * j + 4)),
      label + ': getCorrectiveTerms(' + ord + ')');
  });
  T.check(T.sameBits(index.vectorValue(untouched.ord), untouched.row), label + ': a row that was not named is unchanged');
}

want.cases.forEach(function (c) {
  const g = T.loadGolden(c.name), io = T.inputs(g);
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
  const block = c.frm.map(function (f) { return io.base[f]; });
  const index = fmt.quantizeVectors(io.base).quantizedVectors;
  if (sharded) {
    fmt.searchNearestNeighbors(io.queries[0], index, 5);
    const msg = thrown(function () { fmt.updateVectors(index, c.ords, block); });
    T.check(msg !== null && /not supported on a multi-device index/.test(msg), c.name + ': a multi-device index refuses an update (' + msg + ')');
    T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[c.before[0].q], index, c.before[0].k), c.before[0]), c.name + ': the refused update changed nothing');
    index.dispose();
    return;
  }
  let free = 3; while (c.ords.indexOf(free) >= 0) free++;
  const untouched = { ord: free, row: Uint8Array.from(index.vectorValue(free)) };
  c.before.forEach(function (w) {
    T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[w.q], index, w.k), w), c.name + ' q' + w.q + ' k=' + w.k + ': top-k before updateVectors');
  });
  const even = g.ib === 1 ? bbq.createRowFilter(index, function (i) { return i % 2 === 0; }) : null;  // made before the update
  T.check(fmt.updateVectors(index, c.ords, block) === index, c.name + ': updateVectors returns targetVectors');
  T.check(index.size() === g.n, c.name + ': size() ' + index.size());
  sameRows(index, c, untouched, c.name);
  c.after.forEach(function (w) {
    T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[w.q], index, w.k), w), c.name + ' q' + w.q + ' k=' + w.k + ': top-k after updateVectors');
  });
  const ks = Array.from(new Set(c.after.map(function (w) { return w.k; })));
  ks.forEach(function (k) {
    const batch = fmt.searchNearestNeighborsBatch(io.queries, index, k);
    c.after.filter(function (w) { return w.k === k; }).forEach(function (w) { T.check(sameAnswer(batch[w.q], w), c.name + ' q' + w.q + ' k=' + k + ': batch'); });
  });
  if (even) {
    c.filtered.forEach(function (w) {
      T.check(sameAnswer(fmt.searchNearestNeighborsFiltered(io.queries[w.q], index, even, w.k), w), c.name + ' q' + w.q + ': the filter made before the update still serves');
    });
    even.dispose();
  }
  // an Int32Array of ords, and the same block once more: nothing changes
  fmt.updateVectors(index, Int32Array.from(c.ords), block);
  sameRows(index, c, untouched, c.name + ' twice');
  // a set that has not been searched yet (with the host quantizer: no device copy exists, the host rows alone are patched)
  const cold = fmt.quantizeVectors(io.base).quantizedVectors;
  fmt.updateVectors(cold, c.ords, block);
  sameRows(cold, c, untouched, c.name + ' cold');
  T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[c.after[1].q], cold, c.after[1].k), c.after[1]), c.name + ': cold top-k');
  cold.dispose();
  // validation as appendVectors', and nothing changes on an error
  T.check(thrown(function () { fmt.updateVectors(null, c.ords, block); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.updateVectors(index, [1], [new Float32Array(g.dim + 1)]); }) !== null, 'dimension');
  T.check(thrown(function () { fmt.updateVectors(index, [1, 2], [block[0]]); }) !== null, 'one ord per vector');
  [-1, g.n, 1.5].forEach(function (o) {
    T.check(thrown(function () { fmt.updateVectors(index, [0, o], [block[0], block[1]]); }) === '向量索引 ' + o + ' 不存在', c.name + ': ord ' + o + ' is refused');
  });
  const bad = [Float32Array.from(block[0]), Float32Array.from(block[1])]; bad[1][0] = NaN;
  const msg = thrown(function () { fmt.updateVectors(index, [free, 0], bad); });
  T.check(msg !== null && /向量 1 位置 0 包含NaN值/.test(msg), c.name + ': NaN is refused with its position (' + msg + ')');
  T.check(fmt.updateVectors(index, [], []) === index && index.size() === g.n, c.name + ': an empty block');
  sameRows(index, c, untouched, c.name + ' after refusals');
  T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[c.after[1].q], index, c.after[1].k), c.after[1]), c.name + ': top-k after refusals');
  // a loaded index fetches its host copies lazily: after an update they hold the new rows
  const prefix = path.join(dir, c.name);
  const part = fmt.quantizeVectors(io.base).quantizedVectors;
  fmt.saveIndex(part, prefix);
  part.dispose();
  const loaded = fmt.loadIndex(prefix);
  fmt.updateVectors(loaded, c.ords, block);
  sameRows(loaded, c, untouched, c.name + ' loaded');
  T.check(sameAnswer(fmt.searchNearestNeighbors(io.queries[c.after[0].q], loaded, c.after[0].k), c.after[0]), c.name + ': loaded + updated top-k');
  loaded.dispose();
  // the fp32 side of the rerank recipe follows
  if (g.ib === 1 && g.sim === 'COSINE') {
    const updated = io.base.slice();
    c.ords.forEach(function (o, i) { updated[o] = block[i]; });
    const dv = bbq.createDeviceVectors(io.base), whole = bbq.createDeviceVectors(updated);
    T.check(dv.update(c.ords, block) === dv && dv.length === g.n, c.name + ': DeviceVectors.update');
    const x = bbq.getOversampledTopKWithHeap(io.queries[0], index, dv, 10, 3, fmt), y = bbq.getOversampledTopKWithHeap(io.queries[0], index, whole, 10, 3, fmt);
    T.check(JSON.stringify(x) === JSON.stringify(y) && x.length === 10, c.name + ': rerank over updated vectors');
    const rows = c.ords.concat([free]);
    T.check(T.sameBits(dv.trueScores(io.queries[0], rows), whole.trueScores(io.queries[0], rows)), c.name + ': true scores of updated rows');
    T.check(thrown(function () { dv.update([g.n], [block[0]]); }) === '向量索引 ' + g.n + ' 不存在', c.name + ': DeviceVectors.update refuses an ord outside');
    dv.dispose(); whole.dispose();
  }
  index.dispose();
});
T.finish('gpu_update' + (sharded ? ' (sharded)' : '') + (hostQuantizer ? ' (host quantizer)' : ''));
