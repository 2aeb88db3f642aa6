'use strict';
// GPU: the filtered search of the JavaScript host (createRowFilter, searchNearestNeighborsFiltered, searchNearestNeighborsBatchFiltered)
// against answers the ctypes binding gave for the same fixtures, masks and k (argv[2]: the JSON tests/test_js_filtered.py wrote).
// With BBQ_DEVICES set (a multi-device index) the calls must throw the library's unsupported message instead.
const fs = require('fs');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const want = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
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
  const index = fmt.quantizeVectors(io.base).quantizedVectors;
  const mask = T.dec(c.mask_u8, Uint8Array), ords = [];
  for (let i = 0; i < mask.length; i++) if (mask[i]) ords.push(i);
  if (sharded) {
    const msg = thrown(function () { bbq.createRowFilter(index, mask); });
    T.check(msg !== null && /not supported on a multi-device index/.test(msg), c.name + ': a multi-device index refuses a filter (' + msg + ')');
    index.dispose();
    return;
  }
  // the three forms of `accept`, plus a plain array of ords, shuffled and with duplicates
  const shuffled = ords.concat(ords.slice(0, 7)).reverse();
  const filters = { mask: bbq.createRowFilter(index, mask), ords: bbq.createRowFilter(index, Int32Array.from(ords)),
    array: bbq.createRowFilter(index, shuffled), predicate: bbq.createRowFilter(index, function (ord) { return mask[ord] !== 0; }) };
  Object.keys(filters).forEach(function (form) {
    const f = filters[form];
    T.check(f.count === ords.length, c.name + ' ' + form + ': count ' + f.count);
    c.answers.forEach(function (a) {
      T.check(sameAnswer(fmt.searchNearestNeighborsFiltered(io.queries[a.q], index, f, a.k), a), c.name + ' ' + form + ' q' + a.q + ' k=' + a.k + ': filtered top-k');
    });
  });
  // the batch method: every query of the fixture at once equals the single calls
  const ks = Array.from(new Set(c.answers.map(function (a) { return a.k; })));
  ks.forEach(function (k) {
    const batch = fmt.searchNearestNeighborsBatchFiltered(io.queries, index, filters.mask, k);
    T.check(batch.length === io.queries.length, c.name + ' k=' + k + ': one answer per query');
    c.answers.filter(function (a) { return a.k === k; }).forEach(function (a) {
      T.check(sameAnswer(batch[a.q], a), c.name + ' q' + a.q + ' k=' + k + ': batch');
    });
  });
  // validation: the reference's messages, in searchNearestNeighbors' order
  T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(null, index, filters.mask, 5); }) === '查询向量不能为空', 'null query');
  T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(io.queries[0], null, filters.mask, 5); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(io.queries[0], index, filters.mask, -1); }) === 'k值不能为负数', 'negative k');
  T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(new Float32Array(g.dim + 1), index, filters.mask, 5); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
  T.check(fmt.searchNearestNeighborsFiltered(io.queries[0], index, filters.mask, 0).length === 0, 'k = 0');
  T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(io.queries[0], index, null, 5); }) !== null, 'null filter');
  T.check(thrown(function () { bbq.createRowFilter(index, Int32Array.of(0, g.n)); }) !== null, 'an ord outside the index');
  T.check(thrown(function () { bbq.createRowFilter(index, new Uint8Array(g.n + 1)); }) !== null, 'a mask of the wrong length');
  // dispose: idempotent, and a disposed filter is refused
  Object.keys(filters).forEach(function (form) { filters[form].dispose(); filters[form].dispose(); });
  T.check(thrown(function () { fmt.searchNearestNeighborsFiltered(io.queries[0], index, filters.mask, 5); }) !== null, 'disposed filter');
  index.dispose();
});
T.finish('gpu_filtered' + (sharded ? ' (sharded)' : ''));
