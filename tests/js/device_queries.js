'use strict';
// GPU: quantizeQueriesOnDevice returns the host quantizer's bytes (native.quantizeQueries, the search path) for the queries of the
// README's 1000 x 128 case under every similarity, and its errors are the host's.
const T = require('./common');
const bbq = T.bbq;
if (bbq.deviceCount() < 1) { console.error('no HIP device'); process.exit(2); }

function sameBytes(a, b) {
  if (a.length !== b.length || a.BYTES_PER_ELEMENT !== b.BYTES_PER_ELEMENT) return false;
  const x = new Uint8Array(a.buffer, a.byteOffset, a.byteLength), y = new Uint8Array(b.buffer, b.byteOffset, b.byteLength);
  for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false;
  return true;
}
function thrown(f) { try { f(); } catch (e) { return e.message; } return null; }

const g = T.loadGolden('c1_1000x128_cos_qb4'), io = T.inputs(g);
const SIMS = { EUCLIDEAN: 0, COSINE: 1, MAXIMUM_INNER_PRODUCT: 2 };
Object.keys(SIMS).forEach(function (sim) {
  const fmt = new bbq.BinaryQuantizationFormat({ queryBits: g.qb, indexBits: g.ib, quantizer: { similarityFunction: sim, lambda: g.lambda, iters: g.iters } });
  const index = fmt.quantizeVectors(io.base).quantizedVectors;
  const flat = new Float32Array(io.queries.length * g.dim);
  io.queries.forEach(function (v, i) { flat.set(v, i * g.dim); });
  const want = bbq._native.quantizeQueries(flat, io.queries.length, index.getCentroid(), SIMS[sim], g.qb, g.lambda, g.iters, 2);
  const got = fmt.quantizeQueriesOnDevice(io.queries, index);
  T.check(sameBytes(got.quantized, want.quantized), sim + ' quantized');
  T.check(sameBytes(got.corrections, want.corrections), sim + ' corrections');
  T.check(fmt.quantizeQueriesOnDevice([], index).quantized.length === 0, sim + ' no query');
  const bad = io.queries.slice(0, 3).map(function (v) { return new Float32Array(v); });
  bad[1][5] = NaN;
  const hostMessage = thrown(function () { bbq._native.quantizeQueries(Float32Array.from(bad[1]), 1, index.getCentroid(), SIMS[sim], g.qb, g.lambda, g.iters, 1); });
  T.check(hostMessage !== null && thrown(function () { fmt.quantizeQueriesOnDevice(bad, index); }) === hostMessage, sim + ' NaN message');
  T.check(thrown(function () { fmt.quantizeQueriesOnDevice([new Float32Array(g.dim + 1)], index); }) === '查询向量维度与目标向量维度不匹配', sim + ' dimension');
  index.dispose();
});
T.finish('device_queries');
