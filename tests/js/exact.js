'use strict';
// GPU: the exact search through the JavaScript host - getTrueTopK and DeviceVectors.trueTopK equal the model's answers (argv[2]: the
// JSON tests/test_js_exact.py wrote): the README's 1000 x 128 case, rows that tie, with and without a RowFilter, and the error messages.
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
const index = fmt.quantizeVectors(io.base).quantizedVectors;     // the RowFilter hangs on it
const filter = bbq.createRowFilter(index, T.dec(c.mask_u8, Uint8Array));
const tied = io.base.map(function (v) { return new Float32Array(v); });
c.dups.forEach(function (d) { tied[d[0]] = new Float32Array(io.base[d[1]]); });
const plainV = bbq.createDeviceVectors(io.base), tiedV = bbq.createDeviceVectors(tied);
const queries = io.queries.slice(0, c.nq), tieQueries = [io.queries[0], io.base[7]];

c.cases.forEach(function (a) {
  const label = a.label + ' ' + a.sim + ' k=' + a.k;
  const V = a.tied ? tiedV : plainV, qs = a.tied ? tieQueries : queries;
  const got = V.trueTopK(qs, a.k, a.sim, a.filtered ? filter : undefined);
  let ok = got.length === qs.length;
  for (let q = 0; ok && q < qs.length; q++) {
    const wi = T.dec(a.idx_i32[q], Int32Array), wb = T.dec(a.bits_u64[q], Float64Array);
    ok = sameBytes(Int32Array.from(got[q], function (r) { return r.index; }), wi) && sameBytes(Float64Array.from(got[q], function (r) { return r.trueScore; }), wb);
    if (ok && a.sim === 'COSINE' && !a.filtered) {
      const mine = bbq.getTrueTopK(qs[q], V, a.k);
      ok = Array.isArray(mine) && sameBytes(Int32Array.from(mine), wi);
    }
  }
  T.check(ok, label);
});
// the reference's own shape on host arrays: the same indices
const first = c.cases.filter(function (a) { return a.label === 'plain' && a.sim === 'COSINE' && a.k === 10; })[0];
T.check(sameBytes(Int32Array.from(bbq.getTrueTopK(queries[0], io.base, 10)), T.dec(first.idx_i32[0], Int32Array)), 'getTrueTopK over host rows');
T.check(sameBytes(Int32Array.from(plainV.trueTopK([queries[0]], 10)[0], function (r) { return r.index; }), T.dec(first.idx_i32[0], Int32Array)), 'the default similarity is COSINE');
plainV.setOption('exact_slab_rows', 256);
T.check(sameBytes(Int32Array.from(bbq.getTrueTopK(queries[0], plainV, 10)), T.dec(first.idx_i32[0], Int32Array)), 'exact_slab_rows 256');
T.check(thrown(function () { plainV.setOption('exact_slab_rows', 100); }) !== null, 'a slab that is no multiple of 256');
T.check(thrown(function () { plainV.setOption('exact_slab_cols', 256); }) !== null, 'an unknown option');
plainV.setOption('exact_slab_rows', 0);
T.check(plainV.trueTopK(queries, 0).every(function (r) { return r.length === 0; }), 'k = 0');
T.check(plainV.trueTopK([], 5).length === 0, 'no query');
T.check(thrown(function () { plainV.trueTopK(queries, -1); }) === 'k值不能为负数', 'negative k');
T.check(thrown(function () { plainV.trueTopK(null, 1); }) === '查询向量不能为空', 'null queries');
T.check(thrown(function () { plainV.trueTopK([new Float32Array(g.dim + 1)], 1); }) === '向量维度不匹配', 'dimension');
T.check(thrown(function () { plainV.trueTopK(queries, 1, 'MANHATTAN'); }) !== null, 'an unknown similarity');
T.check(thrown(function () { plainV.trueTopK(queries, 1, 'COSINE', {}); }) !== null, 'a filter that is none');
filter.dispose();
T.check(thrown(function () { plainV.trueTopK(queries, 1, 'COSINE', filter); }) !== null, 'a disposed filter');
plainV.dispose();
tiedV.dispose();
index.dispose();
T.finish('exact');
