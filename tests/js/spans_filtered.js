'use strict';
// GPU: filtered span search through the JavaScript host - searchNearestNeighborsInSpansFiltered equals the oracle's heap over the golden
// scores of the accepted rows of each span set (argv[2]: the JSON tests/test_js_spans_filtered.py wrote) and searchNearestNeighborsFiltered
// when one span covers everything.
const fs = require('fs');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const want = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function sameAnswer(res, b64i, b64s) {
  const wi = T.dec(b64i, Int32Array), ws = T.dec(b64s, Float32Array);
  let ok = res.length === wi.length;
  for (let i = 0; ok && i < res.length; i++) ok = res[i].index === wi[i] && res[i].score === ws[i];
  return ok;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }

want.cases.forEach(function (c) {
  const g = T.loadGolden(c.name), io = T.inputs(g);
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
  const index = fmt.quantizeVectors(io.base).quantizedVectors;
  const filters = {};
  Object.keys(c.masks).forEach(function (m) { filters[m] = bbq.createRowFilter(index, T.dec(c.masks[m], Uint8Array)); });
  let nonEmpty = 0;
  c.answers.forEach(function (a) {
    const label = c.name + ' ' + a.mask + ' q' + a.q + ' k=' + a.k + ' spans ' + JSON.stringify(a.spans).slice(0, 60);
    const res = fmt.searchNearestNeighborsInSpansFiltered(io.queries[a.q], index, a.spans, filters[a.mask], a.k);
    T.check(sameAnswer(res, a.idx_i32, a.score_f32), label);
    if (a.mask === 'none') T.check(res.length === 0, label + ': nothing accepted');
    if (res.length) nonEmpty++;
  });
  T.check(nonEmpty > 0, c.name + ': some answer holds a row');
  const f = filters.drop_every_third, q0 = io.queries[0];
  const flat = new Float64Array([0, g.n]);
  const whole = fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, g.n]], f, 10), byFilter = fmt.searchNearestNeighborsFiltered(q0, index, f, 10);
  T.check(whole.length === 10 && JSON.stringify(whole) === JSON.stringify(byFilter), 'one span over everything is searchNearestNeighborsFiltered');
  T.check(JSON.stringify(fmt.searchNearestNeighborsInSpansFiltered(q0, index, flat, f, 10)) === JSON.stringify(byFilter), 'the same as a Float64Array');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(null, index, [[0, 5]], f, 3); }) === '查询向量不能为空', 'null query');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, null, [[0, 5]], f, 3); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, 5]], f, -1); }) === 'k值不能为负数', 'negative k');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, null, f, 3); }) !== null, 'null spans');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, 5]], null, 3); }) !== null, 'null filter');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, 5]], new Uint8Array(g.n), 3); }) !== null, 'a mask is no RowFilter');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(new Float32Array(g.dim + 1), index, [[0, 5]], f, 3); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
  const overlap = thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, 10], [5, 20]], f, 3); });
  T.check(overlap !== null && overlap.indexOf('query 0, span 1') >= 0 && overlap.indexOf('bbq_search_spans_filtered_batch') >= 0, 'overlapping spans: the message names the span');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, g.n + 1]], f, 3); }) !== null, 'a span beyond the index');
  T.check(fmt.searchNearestNeighborsInSpansFiltered(q0, index, [], f, 3).length === 0, 'no spans: no rows');
  T.check(fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, 5]], f, 0).length === 0, 'k = 0');
  Object.keys(filters).forEach(function (m) { filters[m].dispose(); });
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpansFiltered(q0, index, [[0, 5]], f, 3); }) !== null, 'a disposed filter');
  index.dispose();
});
T.finish('spans_filtered');
