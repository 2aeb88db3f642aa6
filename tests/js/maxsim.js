'use strict';
// GPU: MaxSim search through the JavaScript host - searchNearestNeighborsMaxSim equals the model's answers (argv[2]: the JSON
// tests/test_js_maxsim.py wrote) with the fixture's first queries as one query's token vectors, with and without a row filter, and the
// error messages.
const fs = require('fs');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const c = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function sameAnswer(res, b64g, b64s) {
  const wg = T.dec(b64g, Int32Array), ws = T.dec(b64s, Float32Array);
  let ok = res.length === wg.length;
  for (let i = 0; ok && i < res.length; i++) ok = res[i].group === wg[i] && res[i].score === ws[i];
  return ok;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }

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
  const label = c.name + ' ' + a.layout + ' ' + a.mask + ' tokens=' + a.tokens + ' k=' + a.k;
  const res = fmt.searchNearestNeighborsMaxSim(io.queries.slice(0, a.tokens), index, sets[a.layout + '/' + a.mask], a.k);
  T.check(sameAnswer(res, a.group_i32, a.score_f32), label);
  if (a.mask === 'none') T.check(res.length === 0, label + ': nothing accepted');
  if (res.length) nonEmpty++;
});
T.check(nonEmpty > 0, 'some answer holds a group');
const gs = sets['random_1_20/all'], q0 = io.queries[0];
const one = fmt.searchNearestNeighborsMaxSim([q0], index, gs, 10), grouped = fmt.searchNearestNeighborsGrouped(q0, index, gs, 10);
T.check(one.length === 10 && JSON.stringify(one.map(function (r) { return [r.group, r.score]; })) === JSON.stringify(grouped.map(function (r) { return [r.group, r.score]; })),
        'one vector is searchNearestNeighborsGrouped');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim(null, index, gs, 3); }) === '查询向量不能为空', 'null query');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([], index, gs, 3); }) === '查询向量不能为空', 'no vector');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([q0, null], index, gs, 3); }) === '查询向量不能为空', 'a null vector');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([q0], null, gs, 3); }) === '目标向量集合不能为空', 'null target');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([q0], index, gs, -1); }) === 'k值不能为负数', 'negative k');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([q0], index, null, 3); }) !== null, 'null groups');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([q0, new Float32Array(g.dim + 1)], index, gs, 3); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
T.check(fmt.searchNearestNeighborsMaxSim([q0], index, gs, 0).length === 0, 'k = 0');
Object.keys(sets).forEach(function (s) { sets[s].dispose(); });
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSim([q0], index, gs, 3); }) !== null, 'a disposed group set');
index.dispose();
T.finish('maxsim');
