'use strict';
// GPU: range search through the JavaScript host - searchRange equals the answers the ctypes binding gave for the same fixture, thresholds
// and filter (argv[2]: the JSON tests/test_js_range.py wrote), in ascending ord and by descending score.
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
  const filter = bbq.createRowFilter(index, T.dec(c.mask_u8, Uint8Array));
  let nonEmpty = 0;
  c.answers.forEach(function (a) {
    const t = T.dec(a.threshold_f32, Float32Array)[0], label = c.name + ' q' + a.q + ' t=' + t + (a.filtered ? ' filtered' : '');
    const opt = a.filtered ? { rowFilter: filter } : undefined;
    const byOrd = fmt.searchRange(io.queries[a.q], index, t, opt);
    T.check(sameAnswer(byOrd, a.idx_i32, a.score_f32), label + ': ascending ord');
    T.check(sameAnswer(fmt.searchRange(io.queries[a.q], index, t, { rowFilter: a.filtered ? filter : null, order: 'ord' }), a.idx_i32, a.score_f32), label + ": order 'ord'");
    T.check(sameAnswer(fmt.searchRange(io.queries[a.q], index, t, { rowFilter: a.filtered ? filter : null, order: 'score' }), a.by_score_idx_i32, a.by_score_f32),
      label + ': descending score, ties in ascending ord');
    if (byOrd.length) nonEmpty++;
  });
  T.check(nonEmpty > 0, c.name + ': some answer holds a row');
  T.check(thrown(function () { fmt.searchRange(null, index, 0.5); }) === '查询向量不能为空', 'null query');
  T.check(thrown(function () { fmt.searchRange(io.queries[0], null, 0.5); }) === '目标向量集合不能为空', 'null target');
  T.check(thrown(function () { fmt.searchRange(io.queries[0], index, NaN); }) === '阈值不能为NaN', 'a NaN threshold');
  T.check(thrown(function () { fmt.searchRange(new Float32Array(g.dim + 1), index, 0.5); }) === '查询向量维度与目标向量维度不匹配', 'dimension');
  T.check(thrown(function () { fmt.searchRange(io.queries[0], index, 0.5, { order: 'best' }); }) !== null, 'an order that does not exist');
  T.check(thrown(function () { fmt.searchRange(io.queries[0], index, 0.5, { rowFilter: [1, 2] }); }) !== null, 'a filter that is no RowFilter');
  T.check(fmt.searchRange(io.queries[0], index, Infinity).length === 0, 't = +inf: no finite score reaches it');
  filter.dispose();
  index.dispose();
});
T.finish('range');
