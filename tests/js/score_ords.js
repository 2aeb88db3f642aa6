'use strict';
// GPU: scoring chosen rows through the JavaScript host - computeBatchQuantizedScores over a scattered list equals per-ord calls, and
// searchNearestNeighborsInOrds equals the answers the ctypes binding gave for the same fixture, lists and k (argv[2]: the JSON
// tests/test_js_score_ords.py wrote).  With BBQ_DEVICES set the index is row-sharded: the answers must not change by a bit.
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
function same(a, b) { return a === b || (a !== a && b !== b); }

want.cases.forEach(function (c) {
  const g = T.loadGolden(c.name), io = T.inputs(g), n = g.n;
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
  const index = fmt.quantizeVectors(io.base).quantizedVectors, scorer = fmt.getScorer();
  const q = fmt.quantizeQueryVector(io.queries[0], index.getCentroid());
  // a scattered list with a duplicate equals per-ord calls, entry by entry; an Int32Array is taken as well
  const ords = [n - 1, 0, 17, 17];
  [ords, Int32Array.from(ords)].forEach(function (list, form) {
    const batch = scorer.computeBatchQuantizedScores(q.quantizedQuery, q.queryCorrections, index, list, g.qb);
    let ok = batch.length === ords.length;
    for (let i = 0; ok && i < ords.length; i++) {
      const one = scorer.computeBatchQuantizedScores(q.quantizedQuery, q.queryCorrections, index, [ords[i]], g.qb)[0];
      ok = same(one.score, batch[i].score) && one.bitDotProduct === batch[i].bitDotProduct &&
        batch[i].corrections.index.lowerInterval === index.getCorrectiveTerms(ords[i]).lowerInterval;
    }
    T.check(ok, c.name + ': computeBatchQuantizedScores on [n-1, 0, 17, 17] == per-ord calls (form ' + form + ')');
    T.check(same(batch[2].score, batch[3].score), c.name + ': a duplicate is scored once per occurrence');
  });
  T.check(scorer.computeBatchQuantizedScores(q.quantizedQuery, q.queryCorrections, index, [], g.qb).length === 0, c.name + ': empty ords');
  T.check(thrown(function () { scorer.computeBatchQuantizedScores(q.quantizedQuery, q.queryCorrections, index, [3, n, -1], g.qb); }) === '向量索引 ' + n + ' 不存在',
    c.name + ': the first ord that names no row');
  // the search over a list equals the ctypes answer
  c.answers.forEach(function (a) {
    const list = T.dec(a.ords_i32, Int32Array);
    T.check(sameAnswer(fmt.searchNearestNeighborsInOrds(io.queries[a.q], index, list, a.k), a), c.name + ' q' + a.q + ' k=' + a.k + ' list of ' + list.length + ': top-k in ords');
    T.check(sameAnswer(fmt.searchNearestNeighborsInOrds(io.queries[a.q], index, Array.from(list), a.k), a), c.name + ' q' + a.q + ' k=' + a.k + ': a plain array of ords');
  });
  T.check(thrown(function () { fmt.searchNearestNeighborsInOrds(null, index, [1], 5); }) === '查询向量不能为空', 'null query');
  T.check(thrown(function () { fmt.searchNearestNeighborsInOrds(io.queries[0], null, [1], 5); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.searchNearestNeighborsInOrds(io.queries[0], index, [1], -1); }) === 'k值不能为负数', 'negative k');
  T.check(thrown(function () { fmt.searchNearestNeighborsInOrds(new Float32Array(g.dim + 1), index, [1], 5); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
  T.check(fmt.searchNearestNeighborsInOrds(io.queries[0], index, [1, 2], 0).length === 0, 'k = 0');
  T.check(fmt.searchNearestNeighborsInOrds(io.queries[0], index, [], 4).length === 0, 'an empty list');
  T.check(thrown(function () { fmt.searchNearestNeighborsInOrds(io.queries[0], index, [1, n], 5); }) === '向量索引 ' + n + ' 不存在', 'an ord outside the index');
  index.dispose();
});
T.finish('score_ords' + (sharded ? ' (sharded)' : ''));
