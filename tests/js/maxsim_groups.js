'use strict';
// GPU: MaxSim over chosen groups through the JavaScript host - searchNearestNeighborsMaxSimInGroups and computeMaxSimGroupScores equal
// the model's answers (argv[2]: the JSON tests/test_js_maxsim_groups.py wrote) with the fixture's first queries as one query's token
// vectors, over candidate lists ascending, shuffled and with a duplicate, with and without a row filter, and the error messages.
const fs = require('fs');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const c = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function sameAnswer(res, b64g, b64s) {
  const wg = T.dec(b64g, Int32Array), ws = T.dec(b64s, Float32Array);
  let ok = res.length === wg.length;
  for (let i = 0; ok && i < res.length; i++) ok = res[i].group === wg[i] && (res[i].score === ws[i] || (res[i].score !== res[i].score && ws[i] !== ws[i]));
  return ok;
}
function sameScores(got, b64) {
  const w = T.dec(b64, Float32Array);
  let ok = got instanceof Float32Array && got.length === w.length;
  for (let i = 0; ok && i < w.length; i++) ok = got[i] === w[i] || (got[i] !== got[i] && w[i] !== w[i]);
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
let scored = '';
c.answers.forEach(function (a) {
  const label = c.name + ' ' + a.layout + ' ' + a.mask + ' ' + a.list + ' tokens=' + a.tokens + ' k=' + a.k;
  const set = sets[a.layout + '/' + a.mask], tokens = io.queries.slice(0, a.tokens), cand = T.dec(a.cand_i32, Int32Array);
  const res = fmt.searchNearestNeighborsMaxSimInGroups(tokens, index, set, a.k % 2 ? cand : Array.from(cand), a.k);   // both forms of a list
  T.check(sameAnswer(res, a.group_i32, a.score_f32), label);
  const key = a.layout + a.mask + a.list + a.tokens;
  if (key !== scored) {               // the scores do not depend on k: once per list
    scored = key;
    T.check(sameScores(fmt.computeMaxSimGroupScores(tokens, index, set, cand), a.all_f32), label + ': scores');
  }
});
const gs = sets['random_1_20/all'], q0 = io.queries[0], q1 = io.queries[1];
const nGroups = c.layouts.random_1_20.length - 1;
const all = fmt.searchNearestNeighborsMaxSimInGroups([q0, q1], index, gs, Int32Array.from({ length: nGroups }, function (_, i) { return i; }), 10);
T.check(JSON.stringify(all) === JSON.stringify(fmt.searchNearestNeighborsMaxSim([q0, q1], index, gs, 10)), 'every group, ascending, is searchNearestNeighborsMaxSim');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups(null, index, gs, [1], 3); }) === '查询向量不能为空', 'null query');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([], index, gs, [1], 3); }) === '查询向量不能为空', 'no vector');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], null, gs, [1], 3); }) === '目标向量集合不能为空', 'null target');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], index, gs, [1], -1); }) === 'k值不能为负数', 'negative k');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], index, null, [1], 3); }) !== null, 'null groups');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], index, gs, null, 3); }) === '候选分组不能为空', 'null candidates');
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0, new Float32Array(g.dim + 1)], index, gs, [1], 3); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
T.check(fmt.searchNearestNeighborsMaxSimInGroups([q0], index, gs, [1, 2], 0).length === 0, 'k = 0');
T.check(fmt.searchNearestNeighborsMaxSimInGroups([q0], index, gs, [], 3).length === 0 && fmt.computeMaxSimGroupScores([q0], index, gs, []).length === 0, 'no candidate');
const outside = thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], index, gs, [3, nGroups, 1], 3); });
T.check(outside !== null && outside.indexOf('query 0, position 1: group ' + nGroups) >= 0, 'a group number outside the set names its position: ' + outside);
T.check(thrown(function () { fmt.computeMaxSimGroupScores([q0], index, gs, [3, -1]); }) !== null, 'a negative group number');
Object.keys(c.dead).forEach(function (l) {
  const m = thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], index, sets[l + '/drop_every_third'], [c.dead[l]], 3); });
  T.check(m !== null && m.indexOf('not live') >= 0, l + ': a group without an accepted row: ' + m);
});
Object.keys(sets).forEach(function (s) { sets[s].dispose(); });
T.check(thrown(function () { fmt.searchNearestNeighborsMaxSimInGroups([q0], index, gs, [1], 3); }) !== null, 'a disposed group set');
index.dispose();
T.finish('maxsim_groups');
