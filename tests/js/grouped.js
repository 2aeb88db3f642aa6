'use strict';
// GPU: grouped search through the JavaScript host - searchNearestNeighborsGrouped equals the oracle's heap over the golden scores of each
// live group's representative (argv[2]: the JSON tests/test_js_grouped.py wrote), with and without a row filter, and the error messages.
const fs = require('fs');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const want = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function sameAnswer(res, b64i, b64g, b64s) {
  const wi = T.dec(b64i, Int32Array), wg = T.dec(b64g, Int32Array), ws = T.dec(b64s, Float32Array);
  let ok = res.length === wi.length;
  for (let i = 0; ok && i < res.length; i++) ok = res[i].index === wi[i] && res[i].group === wg[i] && res[i].score === ws[i];
  return ok;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }

want.cases.forEach(function (c) {
  const g = T.loadGolden(c.name), io = T.inputs(g);
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
  const index = fmt.quantizeVectors(io.base).quantizedVectors;
  const sets = {};
  Object.keys(c.layouts).forEach(function (l) {
    Object.keys(c.masks).forEach(function (m) {
      if (m === 'all') { sets[l + '/' + m] = bbq.createRowGroups(index, c.layouts[l]); return; }
      const f = bbq.createRowFilter(index, T.dec(c.masks[m], Uint8Array));
      sets[l + '/' + m] = bbq.createRowGroups(index, Float64Array.from(c.layouts[l]), f);
      f.dispose();                      // the group set keeps its own copy of the filter's words
    });
  });
  let nonEmpty = 0;
  c.answers.forEach(function (a) {
    const label = c.name + ' ' + a.layout + ' ' + a.mask + ' q' + a.q + ' k=' + a.k;
    const gs = sets[a.layout + '/' + a.mask];
    T.check(gs.live === a.live && gs.count === c.layouts[a.layout].length - 1, label + ': count and live');
    const res = fmt.searchNearestNeighborsGrouped(io.queries[a.q], index, gs, a.k);
    T.check(sameAnswer(res, a.idx_i32, a.group_i32, a.score_f32), label);
    if (a.mask === 'none') T.check(res.length === 0, label + ': nothing accepted');
    if (res.length) nonEmpty++;
  });
  T.check(nonEmpty > 0, c.name + ': some answer holds a row');
  const gs = sets['random_1_20/all'], q0 = io.queries[0];
  const single = fmt.searchNearestNeighborsGrouped(q0, index, sets['singletons/all'], 10), plain = fmt.searchNearestNeighbors(q0, index, 10);
  T.check(single.length === 10 && JSON.stringify(single.map(function (r) { return [r.index, r.score]; })) === JSON.stringify(plain.map(function (r) { return [r.index, r.score]; })),
          'all singletons is searchNearestNeighbors');
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(null, index, gs, 3); }) === '查询向量不能为空', 'null query');
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(q0, null, gs, 3); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(q0, index, gs, -1); }) === 'k值不能为负数', 'negative k');
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(q0, index, null, 3); }) !== null, 'null groups');
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(q0, index, c.layouts.one_group, 3); }) !== null, 'offsets are no RowGroups');
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(new Float32Array(g.dim + 1), index, gs, 3); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
  T.check(fmt.searchNearestNeighborsGrouped(q0, index, gs, 0).length === 0, 'k = 0');
  const descending = thrown(function () { bbq.createRowGroups(index, [0, 600, 500, g.n]); });
  T.check(descending !== null && descending.indexOf('bbq_groups_create') >= 0 && descending.indexOf('ascend') >= 0, 'descending offsets: the library\'s message');
  T.check(thrown(function () { bbq.createRowGroups(index, [1, g.n]); }) !== null, 'offsets that do not start at 0');
  T.check(thrown(function () { bbq.createRowGroups(index, [0, g.n - 1]); }) !== null, 'offsets that do not end at size()');
  T.check(thrown(function () { bbq.createRowGroups(index, [0, 0.5, g.n]); }) !== null, 'offsets are integers');
  T.check(thrown(function () { bbq.createRowGroups(index, null); }) !== null, 'null offsets');
  T.check(thrown(function () { bbq.createRowGroups(index, [0, g.n], new Uint8Array(g.n)); }) !== null, 'a mask is no RowFilter');
  T.check(thrown(function () { bbq.createRowGroups(null, [0, g.n]); }) === '目标向量集合不能为空', 'null target at creation');
  Object.keys(sets).forEach(function (s) { sets[s].dispose(); });
  T.check(thrown(function () { fmt.searchNearestNeighborsGrouped(q0, index, gs, 3); }) !== null, 'a disposed group set');
  index.dispose();
});
T.finish('grouped');
