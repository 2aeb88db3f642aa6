'use strict';
// GPU: the exact MaxSim rerank through the JavaScript host - computeMaxSimGroupTrueScores and getOversampledMaxSimTopK equal, byte for
// byte, the answers the ctypes binding gave (argv[2]: the JSON tests/test_js_maxsim_rerank.py wrote) with the fixture's first queries as
// one query's token vectors, and the error messages.
const fs = require('fs');
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }
const c = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function sameBytes(a, b) {
  if (a.length !== b.length || a.BYTES_PER_ELEMENT !== b.BYTES_PER_ELEMENT) return false;
  const x = new Uint8Array(a.buffer, a.byteOffset, a.byteLength), y = new Uint8Array(b.buffer, b.byteOffset, b.byteLength);
  for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false;
  return true;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }

const g = T.loadGolden(c.name), io = T.inputs(g);
const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: g.sim, lambda: g.lambda, iters: g.iters } });
const index = fmt.quantizeVectors(io.base).quantizedVectors;
const vectors = bbq.createDeviceVectors(io.base);
const groups = bbq.createRowGroups(index, c.layout);
const tokens = io.queries.slice(0, c.tokens), cand = T.dec(c.cand_i32, Int32Array);

Object.keys(c.true_f64).forEach(function (sim) {
  const got = bbq.computeMaxSimGroupTrueScores(tokens, vectors, groups, sim === 'COSINE' ? cand : Array.from(cand), sim);   // both forms of a list
  T.check(got instanceof Float64Array && sameBytes(got, T.dec(c.true_f64[sim], Float64Array)), 'computeMaxSimGroupTrueScores ' + sim);
});
T.check(sameBytes(bbq.computeMaxSimGroupTrueScores(tokens, vectors, groups, cand), T.dec(c.true_f64.COSINE, Float64Array)), 'the default similarity is COSINE');
c.recipe.forEach(function (a) {
  const label = 'getOversampledMaxSimTopK k=' + a.k + ' factor=' + a.factor + ' ' + a.selector;
  const res = bbq.getOversampledMaxSimTopK(tokens, index, vectors, groups, a.k, a.factor, fmt, a.selector);
  const wg = T.dec(a.group_i32, Int32Array), wq = T.dec(a.quant_f32, Float32Array), wt = T.dec(a.true_f64, Float64Array);
  let ok = res.length === wg.length;
  for (let i = 0; ok && i < res.length; i++) {
    ok = res[i].group === wg[i] && sameBytes(Float32Array.of(res[i].quantizedScore), wq.subarray(i, i + 1)) && sameBytes(Float64Array.of(res[i].trueScore), wt.subarray(i, i + 1));
  }
  T.check(ok, label);
});
const q0 = io.queries[0], nGroups = c.layout.length - 1;
T.check(bbq.getOversampledMaxSimTopK([q0], index, vectors, groups, 0, 3, fmt).length === 0, 'k = 0');
T.check(bbq.computeMaxSimGroupTrueScores([q0], vectors, groups, []).length === 0, 'no candidate');
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores(null, vectors, groups, [1]); }) === '查询向量不能为空', 'null query');
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores([q0], io.base, groups, [1]); }) !== null, 'host vectors');
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores([q0], vectors, null, [1]); }) !== null, 'null groups');
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores([q0], vectors, groups, null); }) === '候选分组不能为空', 'null candidates');
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores([new Float32Array(g.dim + 1)], vectors, groups, [1]); }) === '向量维度不匹配', 'dimension');
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores([q0], vectors, groups, [1], 'MANHATTAN'); }) !== null, 'an unknown similarity');
const outside = thrown(function () { bbq.computeMaxSimGroupTrueScores([q0], vectors, groups, [3, nGroups, 1]); });
T.check(outside !== null && outside.indexOf('query 0, position 1: group ' + nGroups) >= 0, 'a group number outside the set names its position: ' + outside);
T.check(thrown(function () { bbq.getOversampledMaxSimTopK([q0], index, vectors, groups, -1, 3, fmt); }) === 'k值不能为负数', 'negative k');
T.check(thrown(function () { bbq.getOversampledMaxSimTopK([q0], index, vectors, groups, 3, 0, fmt); }) !== null, 'factor 0');
T.check(thrown(function () { bbq.getOversampledMaxSimTopK([q0], null, vectors, groups, 3, 3, fmt); }) === '目标向量集合不能为空', 'null target');
groups.dispose();
T.check(thrown(function () { bbq.computeMaxSimGroupTrueScores([q0], vectors, groups, [1]); }) !== null, 'a disposed group set');
vectors.dispose();
index.dispose();
T.finish('maxsim_rerank');
