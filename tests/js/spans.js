'use strict';
// GPU: span search through the JavaScript host - searchNearestNeighborsInSpans equals the oracle's heap over the golden scores of the rows
// of each span set (argv[2]: the JSON tests/test_js_spans.py wrote).
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
  let nonEmpty = 0;
  c.answers.forEach(function (a) {
    const label = c.name + ' q' + a.q + ' k=' + a.k + ' spans ' + JSON.stringify(a.spans).slice(0, 60);
    const res = fmt.searchNearestNeighborsInSpans(io.queries[a.q], index, a.spans, a.k);
    T.check(sameAnswer(res, a.idx_i32, a.score_f32), label);
    const flat = new Float64Array(2 * a.spans.length);
    a.spans.forEach(function (s, i) { flat[2 * i] = s[0]; flat[2 * i + 1] = s[1]; });
    T.check(sameAnswer(fmt.searchNearestNeighborsInSpans(io.queries[a.q], index, flat, a.k), a.idx_i32, a.score_f32), label + ': as a Float64Array');
    if (res.length) nonEmpty++;
  });
  T.check(nonEmpty > 0, c.name + ': some answer holds a row');
  const whole = fmt.searchNearestNeighborsInSpans(io.queries[0], index, [[0, g.n]], 10), plain = fmt.searchNearestNeighbors(io.queries[0], index, 10);
  T.check(JSON.stringify(whole) === JSON.stringify(plain), 'one span over everything is searchNearestNeighbors');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(null, index, [[0, 5]], 3); }) === '查询向量不能为空', 'null query');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(io.queries[0], null, [[0, 5]], 3); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(io.queries[0], index, [[0, 5]], -1); }) === 'k值不能为负数', 'negative k');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(io.queries[0], index, null, 3); }) !== null, 'null spans');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(new Float32Array(g.dim + 1), index, [[0, 5]], 3); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
  const overlap = thrown(function () { fmt.searchNearestNeighborsInSpans(io.queries[0], index, [[0, 10], [5, 20]], 3); });
  T.check(overlap !== null && overlap.indexOf('query 0, span 1') >= 0, 'overlapping spans: the message names the span');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(io.queries[0], index, [[0, g.n + 1]], 3); }) !== null, 'a span beyond the index');
  T.check(thrown(function () { fmt.searchNearestNeighborsInSpans(io.queries[0], index, [[0.5, 3]], 3); }) !== null, 'a span that is no pair of integers');
  T.check(fmt.searchNearestNeighborsInSpans(io.queries[0], index, [], 3).length === 0, 'no spans: no rows');
  T.check(fmt.searchNearestNeighborsInSpans(io.queries[0], index, [[0, 5]], 0).length === 0, 'k = 0');
  index.dispose();
});
T.finish('spans');
