/*
 * bbq_napi.c - thin Node N-API (v8, plain C, no node-addon-api) binding of libbbq's C ABI (include/bbq.h).
 * The JavaScript host (../js/index.js) keeps the reference's public API and calls these functions; typed arrays
 * are passed zero-copy (napi_get_typedarray_info) and are only valid for the duration of the call, exactly as
 * the C ABI borrows them.  Errors become JS `Error`s carrying bbq_last_error() (the reference's own messages).
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/bbq.h"

#define NAPI_CALL(env, call)                                              \
  do {                                                                    \
    if ((call) != napi_ok) {                                              \
      napi_throw_error((env), NULL, "bbq_napi: N-API call failed: " #call); \
      return NULL;                                                        \
    }                                                                     \
  } while (0)

static napi_value throw_bbq(napi_env env, int rc) {
  char code[16];
  snprintf(code, sizeof code, "BBQ%d", rc);
  const char *m = bbq_last_error();
  napi_throw_error(env, code, (m && *m) ? m : "libbbq error");
  return NULL;
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
    napi_throw_type_error(env, NULL, "bbq_napi: wrong number of arguments");
    return 0;
  }
  return 1;
}

static int get_typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
  bool is = false;
  napi_typedarray_type t;
  napi_value ab;
  size_t off;
  if (napi_is_typedarray(env, v, &is) != napi_ok || !is ||
      napi_get_typedarray_info(env, v, &t, len, data, &ab, &off) != napi_ok || t != want) {
    napi_throw_type_error(env, NULL, "bbq_napi: typed array of the wrong kind");
    return 0;
  }
  return 1;
}

static int get_i64(napi_env env, napi_value v, int64_t *out) {
  double d;
  if (napi_get_value_double(env, v, &d) != napi_ok) {
    napi_throw_type_error(env, NULL, "bbq_napi: number expected");
    return 0;
  }
  *out = (int64_t)d;
  return 1;
}
static int get_f64(napi_env env, napi_value v, double *out) {
  if (napi_get_value_double(env, v, out) != napi_ok) {
    napi_throw_type_error(env, NULL, "bbq_napi: number expected");
    return 0;
  }
  return 1;
}

static napi_value new_typed(napi_env env, napi_typedarray_type t, size_t count, size_t elem, void **data) {
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, count * elem, data, &ab) != napi_ok) return NULL;
  if (napi_create_typedarray(env, t, count, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}

static void set_prop(napi_env env, napi_value obj, const char *name, napi_value v) { napi_set_named_property(env, obj, name, v); }

/* deviceCount() */
static napi_value DeviceCount(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  NAPI_CALL(env, napi_create_int32(env, bbq_device_count(), &r));
  return r;
}

/* quantizeVectors(flat Float32Array, n, dim, sim, indexBits, lambda, iters, threads) -> {codes, corr, centroid} */
static napi_value QuantizeVectors(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  void *vec; size_t vlen;
  int64_t n, dim, sim, ib, iters, threads; double lambda;
  if (!get_typed(env, a[0], napi_float32_array, &vec, &vlen) || !get_i64(env, a[1], &n) || !get_i64(env, a[2], &dim) ||
      !get_i64(env, a[3], &sim) || !get_i64(env, a[4], &ib) || !get_f64(env, a[5], &lambda) || !get_i64(env, a[6], &iters) ||
      !get_i64(env, a[7], &threads)) return NULL;
  if (n < 0 || dim <= 0 || (size_t)(n * dim) != vlen) { napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the array"); return NULL; }
  const size_t rb = ib == 1 ? (size_t)((dim + 7) / 8) : (size_t)dim;
  void *codes, *corr, *cen;
  napi_value tcodes = new_typed(env, napi_uint8_array, (size_t)n * rb, 1, &codes);
  napi_value tcorr = new_typed(env, napi_float64_array, (size_t)n * 4, 8, &corr);
  napi_value tcen = new_typed(env, napi_float32_array, (size_t)dim, 4, &cen);
  if (!tcodes || !tcorr || !tcen) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_quantize_vectors((const float *)vec, n, (int32_t)dim, (int32_t)sim, (int32_t)ib, lambda, (int32_t)iters, (int32_t)threads,
                                (uint8_t *)codes, (double *)corr, (float *)cen, NULL, NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "codes", tcodes); set_prop(env, o, "corr", tcorr); set_prop(env, o, "centroid", tcen);
  return o;
}

/* quantizeQuery(query Float32Array, centroid Float32Array, sim, queryBits, lambda, iters, searchPath) -> {quantizedQuery, corrections} */
static napi_value QuantizeQuery(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  void *q, *c; size_t ql, cl;
  int64_t sim, qb, iters; double lambda; bool sp;
  if (!get_typed(env, a[0], napi_float32_array, &q, &ql) || !get_typed(env, a[1], napi_float32_array, &c, &cl) ||
      !get_i64(env, a[2], &sim) || !get_i64(env, a[3], &qb) || !get_f64(env, a[4], &lambda) || !get_i64(env, a[5], &iters)) return NULL;
  NAPI_CALL(env, napi_get_value_bool(env, a[6], &sp));
  if (ql != cl) { napi_throw_error(env, "BBQ6", "向量和质心维度不匹配"); return NULL; }
  void *qq, *qc;
  napi_value tqq = new_typed(env, napi_uint8_array, ql, 1, &qq);
  napi_value tqc = new_typed(env, napi_float64_array, 4, 8, &qc);
  if (!tqq || !tqc) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = sp ? bbq_quantize_query((const float *)q, (int32_t)ql, (const float *)c, (int32_t)sim, (int32_t)qb, lambda, (int32_t)iters, (uint8_t *)qq, (double *)qc)
              : bbq_quantize_query_vector((const float *)q, (int32_t)ql, (const float *)c, (int32_t)sim, (int32_t)qb, lambda, (int32_t)iters, (uint8_t *)qq, (double *)qc);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "quantizedQuery", tqq); set_prop(env, o, "corrections", tqc);
  return o;
}

/* centroidDP(centroid Float32Array) */
static napi_value CentroidDP(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  void *c; size_t cl;
  if (!get_typed(env, a[0], napi_float32_array, &c, &cl)) return NULL;
  napi_value r;
  NAPI_CALL(env, napi_create_double(env, bbq_centroid_dp((const float *)c, (int32_t)cl), &r));
  return r;
}

static void finalize_index(napi_env env, void *data, void *hint) {
  (void)env; (void)hint;
  bbq_index **box = (bbq_index **)data;
  if (*box) bbq_index_destroy(*box);
  free(box);
}

static bbq_index *unbox(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || !*(bbq_index **)p) {
    napi_throw_error(env, NULL, "目标向量集合不能为空");
    return NULL;
  }
  return *(bbq_index **)p;
}

/* indexCreate(codes Uint8Array, corr Float64Array, n, dim, indexBits, centroidDP, device) -> external */
static napi_value IndexCreate(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  void *codes, *corr; size_t cl, rl;
  int64_t n, dim, ib, dev; double cdp;
  if (!get_typed(env, a[0], napi_uint8_array, &codes, &cl) || !get_typed(env, a[1], napi_float64_array, &corr, &rl) ||
      !get_i64(env, a[2], &n) || !get_i64(env, a[3], &dim) || !get_i64(env, a[4], &ib) || !get_f64(env, a[5], &cdp) ||
      !get_i64(env, a[6], &dev)) return NULL;
  if (n < 0 || dim <= 0 || rl != (size_t)n * 4 || cl < (size_t)n * (size_t)(ib == 1 ? (dim + 7) / 8 : dim)) {
    napi_throw_range_error(env, NULL, "bbq_napi: array sizes do not match n/dim"); return NULL;
  }
  bbq_index **box = (bbq_index **)calloc(1, sizeof *box);
  int rc = bbq_index_create((const uint8_t *)codes, (const double *)corr, n, (int32_t)dim, (int32_t)ib, cdp, (int32_t)dev, box);
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext;
  if (napi_create_external(env, box, finalize_index, NULL, &ext) != napi_ok) { bbq_index_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  return ext;
}

/* indexCreateMulti(codes Uint8Array, corr Float64Array, n, dim, indexBits, centroidDP, devices Int32Array, pilotRows) -> external
 * one index row-sharded over the listed devices behind one handle (bbq_index_create_multi) */
static napi_value IndexCreateMulti(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  void *codes, *corr, *devs; size_t cl, rl, dl;
  int64_t n, dim, ib, pilot; double cdp;
  if (!get_typed(env, a[0], napi_uint8_array, &codes, &cl) || !get_typed(env, a[1], napi_float64_array, &corr, &rl) ||
      !get_i64(env, a[2], &n) || !get_i64(env, a[3], &dim) || !get_i64(env, a[4], &ib) || !get_f64(env, a[5], &cdp) ||
      !get_typed(env, a[6], napi_int32_array, &devs, &dl) || !get_i64(env, a[7], &pilot)) return NULL;
  if (n < 0 || dim <= 0 || rl != (size_t)n * 4 || cl < (size_t)n * (size_t)(ib == 1 ? (dim + 7) / 8 : dim) || dl < 1) {
    napi_throw_range_error(env, NULL, "bbq_napi: array sizes do not match n/dim"); return NULL;
  }
  bbq_index **box = (bbq_index **)calloc(1, sizeof *box);
  int rc = bbq_index_create_multi((const uint8_t *)codes, (const double *)corr, n, (int32_t)dim, (int32_t)ib, cdp, (int32_t)dl,
                                  (const int32_t *)devs, pilot, box);
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext;
  if (napi_create_external(env, box, finalize_index, NULL, &ext) != napi_ok) { bbq_index_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  return ext;
}

/* indexBuild(flat Float32Array, n, dim, sim, lambda, iters, device, indexBits) -> {handle, codes, corr, centroid}
 * quantizeVectors on the device (bbq_index_build_bits); the handle is the ready device index */
static napi_value IndexBuild(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  void *vec; size_t vlen;
  int64_t n, dim, sim, iters, dev, ib; double lambda;
  if (!get_typed(env, a[0], napi_float32_array, &vec, &vlen) || !get_i64(env, a[1], &n) || !get_i64(env, a[2], &dim) ||
      !get_i64(env, a[3], &sim) || !get_f64(env, a[4], &lambda) || !get_i64(env, a[5], &iters) || !get_i64(env, a[6], &dev) ||
      !get_i64(env, a[7], &ib)) return NULL;
  if (n < 0 || dim <= 0 || (size_t)(n * dim) != vlen) { napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the array"); return NULL; }
  void *codes, *corr, *cen;
  napi_value tcodes = new_typed(env, napi_uint8_array, (size_t)n * (size_t)(ib == 1 ? (dim + 7) / 8 : dim), 1, &codes);
  napi_value tcorr = new_typed(env, napi_float64_array, (size_t)n * 4, 8, &corr);
  napi_value tcen = new_typed(env, napi_float32_array, (size_t)dim, 4, &cen);
  if (!tcodes || !tcorr || !tcen) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  bbq_index **box = (bbq_index **)calloc(1, sizeof *box);
  int rc = bbq_index_build_bits((const float *)vec, n, (int32_t)dim, (int32_t)sim, (int32_t)ib, lambda, (int32_t)iters, (int32_t)dev, box,
                                (float *)cen, (uint8_t *)codes, (double *)corr, NULL, NULL);
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext, o;
  if (napi_create_external(env, box, finalize_index, NULL, &ext) != napi_ok) { bbq_index_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "handle", ext); set_prop(env, o, "codes", tcodes); set_prop(env, o, "corr", tcorr); set_prop(env, o, "centroid", tcen);
  return o;
}

/* quantizeRows(flat Float32Array, n, dim, centroid Float32Array, sim, indexBits, lambda, iters, threads) -> {codes, corr}
 * quantizeVectors' per-row part against a given centroid, on the host (bbq_quantize_rows) */
static napi_value QuantizeRows(napi_env env, napi_callback_info info) {
  napi_value a[9];
  if (!get_args(env, info, 9, a)) return NULL;
  void *vec, *cen; size_t vlen, clen;
  int64_t n, dim, sim, ib, iters, threads; double lambda;
  if (!get_typed(env, a[0], napi_float32_array, &vec, &vlen) || !get_i64(env, a[1], &n) || !get_i64(env, a[2], &dim) ||
      !get_typed(env, a[3], napi_float32_array, &cen, &clen) || !get_i64(env, a[4], &sim) || !get_i64(env, a[5], &ib) ||
      !get_f64(env, a[6], &lambda) || !get_i64(env, a[7], &iters) || !get_i64(env, a[8], &threads)) return NULL;
  if (n < 0 || dim <= 0 || (size_t)(n * dim) != vlen || clen != (size_t)dim) { napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the arrays"); return NULL; }
  void *codes, *corr;
  napi_value tcodes = new_typed(env, napi_uint8_array, (size_t)n * (size_t)(ib == 1 ? (dim + 7) / 8 : dim), 1, &codes);
  napi_value tcorr = new_typed(env, napi_float64_array, (size_t)n * 4, 8, &corr);
  if (!tcodes || !tcorr) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_quantize_rows((const float *)vec, n, (int32_t)dim, (const float *)cen, (int32_t)sim, (int32_t)ib, lambda, (int32_t)iters,
                             (int32_t)threads, (uint8_t *)codes, (double *)corr, NULL, NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "codes", tcodes); set_prop(env, o, "corr", tcorr);
  return o;
}

/* indexAppend(handle, flat Float32Array, n, dim, centroid Float32Array, sim, lambda, iters) -> {codes, corr}
 * raw rows quantized on the device against the index's centroid become its next ords (bbq_index_append) */
static napi_value IndexAppend(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *vec, *cen; size_t vlen, clen;
  int64_t n, dim, sim, iters; double lambda;
  if (!get_typed(env, a[1], napi_float32_array, &vec, &vlen) || !get_i64(env, a[2], &n) || !get_i64(env, a[3], &dim) ||
      !get_typed(env, a[4], napi_float32_array, &cen, &clen) || !get_i64(env, a[5], &sim) || !get_f64(env, a[6], &lambda) ||
      !get_i64(env, a[7], &iters)) return NULL;
  if (n < 0 || dim != bbq_index_dimension(ix) || (size_t)(n * dim) != vlen || clen != (size_t)dim) {
    napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the arrays or the index"); return NULL;
  }
  const int64_t ib = bbq_index_bits(ix);
  void *codes, *corr;
  napi_value tcodes = new_typed(env, napi_uint8_array, (size_t)n * (size_t)(ib == 1 ? (dim + 7) / 8 : dim), 1, &codes);
  napi_value tcorr = new_typed(env, napi_float64_array, (size_t)n * 4, 8, &corr);
  if (!tcodes || !tcorr) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_index_append(ix, (const float *)vec, n, (const float *)cen, (int32_t)sim, lambda, (int32_t)iters, (uint8_t *)codes, (double *)corr, NULL, NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "codes", tcodes); set_prop(env, o, "corr", tcorr);
  return o;
}

/* indexAppendRows(handle, codes Uint8Array, corr Float64Array, n): rows already quantized (bbq_index_append_rows) */
static napi_value IndexAppendRows(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!get_args(env, info, 4, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *codes, *corr; size_t cl, rl;
  int64_t n;
  if (!get_typed(env, a[1], napi_uint8_array, &codes, &cl) || !get_typed(env, a[2], napi_float64_array, &corr, &rl) || !get_i64(env, a[3], &n)) return NULL;
  const int64_t dim = bbq_index_dimension(ix);
  if (n < 0 || rl != (size_t)n * 4 || cl != (size_t)n * (size_t)(bbq_index_bits(ix) == 1 ? (dim + 7) / 8 : dim)) {
    napi_throw_range_error(env, NULL, "bbq_napi: array sizes do not match n/dim"); return NULL;
  }
  int rc = bbq_index_append_rows(ix, (const uint8_t *)codes, (const double *)corr, n);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* indexUpdate(handle, ords Int32Array[n], flat Float32Array, n, dim, centroid Float32Array, sim, lambda, iters) -> {codes, corr}
 * raw rows quantized on the device against the index's centroid replace the rows `ords` in place (bbq_index_update); codes / corr
 * hold all n rows of the block */
static napi_value IndexUpdate(napi_env env, napi_callback_info info) {
  napi_value a[9];
  if (!get_args(env, info, 9, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *ords, *vec, *cen; size_t ol, vlen, clen;
  int64_t n, dim, sim, iters; double lambda;
  if (!get_typed(env, a[1], napi_int32_array, &ords, &ol) || !get_typed(env, a[2], napi_float32_array, &vec, &vlen) || !get_i64(env, a[3], &n) ||
      !get_i64(env, a[4], &dim) || !get_typed(env, a[5], napi_float32_array, &cen, &clen) || !get_i64(env, a[6], &sim) ||
      !get_f64(env, a[7], &lambda) || !get_i64(env, a[8], &iters)) return NULL;
  if (n < 0 || dim != bbq_index_dimension(ix) || (size_t)(n * dim) != vlen || clen != (size_t)dim || ol != (size_t)n) {
    napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the arrays or the index"); return NULL;
  }
  const int64_t ib = bbq_index_bits(ix);
  void *codes, *corr;
  napi_value tcodes = new_typed(env, napi_uint8_array, (size_t)n * (size_t)(ib == 1 ? (dim + 7) / 8 : dim), 1, &codes);
  napi_value tcorr = new_typed(env, napi_float64_array, (size_t)n * 4, 8, &corr);
  if (!tcodes || !tcorr) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_index_update(ix, (const int32_t *)ords, (const float *)vec, n, (const float *)cen, (int32_t)sim, lambda, (int32_t)iters,
                            (uint8_t *)codes, (double *)corr, NULL, NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "codes", tcodes); set_prop(env, o, "corr", tcorr);
  return o;
}

/* indexUpdateRows(handle, ords Int32Array[n], codes Uint8Array, corr Float64Array, n): rows already quantized (bbq_index_update_rows) */
static napi_value IndexUpdateRows(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!get_args(env, info, 5, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *ords, *codes, *corr; size_t ol, cl, rl;
  int64_t n;
  if (!get_typed(env, a[1], napi_int32_array, &ords, &ol) || !get_typed(env, a[2], napi_uint8_array, &codes, &cl) ||
      !get_typed(env, a[3], napi_float64_array, &corr, &rl) || !get_i64(env, a[4], &n)) return NULL;
  const int64_t dim = bbq_index_dimension(ix);
  if (n < 0 || ol != (size_t)n || rl != (size_t)n * 4 || cl != (size_t)n * (size_t)(bbq_index_bits(ix) == 1 ? (dim + 7) / 8 : dim)) {
    napi_throw_range_error(env, NULL, "bbq_napi: array sizes do not match n/dim"); return NULL;
  }
  int rc = bbq_index_update_rows(ix, (const int32_t *)ords, (const uint8_t *)codes, (const double *)corr, n);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* updateWinners(ords Int32Array, rows) -> Float64Array: the positions into the block that take effect, ascending by ord, the last
 * occurrence of every distinct ord (bbq_update_winners; host only) */
static napi_value UpdateWinners(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  void *ords; size_t ol;
  int64_t rows;
  if (!get_typed(env, a[0], napi_int32_array, &ords, &ol) || !get_i64(env, a[1], &rows)) return NULL;
  int64_t *pos = (int64_t *)calloc(ol + 1, sizeof(int64_t)), m = 0;
  if (!pos) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_update_winners((const int32_t *)ords, (int64_t)ol, rows, pos, (int64_t)ol, &m);
  if (rc != BBQ_OK) { free(pos); return throw_bbq(env, rc); }
  void *out;
  napi_value t = new_typed(env, napi_float64_array, (size_t)m, 8, &out);
  if (!t) { free(pos); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  for (int64_t i = 0; i < m; ++i) ((double *)out)[i] = (double)pos[i];
  free(pos);
  return t;
}

/* indexReserve(handle, rows) -> capacity in rows (bbq_index_reserve, bbq_index_capacity) */
static napi_value IndexReserve(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  int64_t rows;
  if (!get_i64(env, a[1], &rows)) return NULL;
  int rc = bbq_index_reserve(ix, rows);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value r;
  NAPI_CALL(env, napi_create_double(env, (double)bbq_index_capacity(ix), &r));
  return r;
}

/* indexDestroy(handle) */
static napi_value IndexDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  void *p = NULL;
  if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
    bbq_index **box = (bbq_index **)p;
    if (*box) { bbq_index_destroy(*box); *box = NULL; }
  }
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* searchBatch(handle, nq, qquant Uint8Array[nq*dim], qcorr Float64Array[nq*4], queryBits, sim, k) -> {indices Int32Array[nq*k], scores Float32Array[nq*k], counts Float64Array[nq]} */
static napi_value SearchBatch(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *qq, *qc; size_t ql, cl;
  int64_t nq, qb, sim, k;
  if (!get_i64(env, a[1], &nq) || !get_typed(env, a[2], napi_uint8_array, &qq, &ql) || !get_typed(env, a[3], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[4], &qb) || !get_i64(env, a[5], &sim) || !get_i64(env, a[6], &k)) return NULL;
  if (nq < 0 || ql != (size_t)nq * (size_t)bbq_index_dimension(ix) || cl != (size_t)nq * 4) {
    napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL;
  }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  int64_t keff = k < bbq_index_size(ix) ? k : bbq_index_size(ix);
  void *oi, *os, *on;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)(nq * keff), 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)(nq * keff), 4, &os);
  napi_value tn = new_typed(env, napi_float64_array, (size_t)nq, 8, &on);
  if (!ti || !ts || !tn) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t *cnt = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
  /* outputs are strided by the k passed to the library: pass keff so rows are packed */
  int rc = bbq_search_batch(ix, (int32_t)nq, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, (int32_t *)oi, (float *)os, cnt);
  if (rc != BBQ_OK) { free(cnt); return throw_bbq(env, rc); }
  for (int64_t i = 0; i < nq; ++i) ((double *)on)[i] = (double)cnt[i];
  free(cnt);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts); set_prop(env, o, "counts", tn);
  napi_value kv; napi_create_double(env, (double)keff, &kv); set_prop(env, o, "stride", kv);
  return o;
}

/* ---- filtered search (bbq_filter_*, bbq_search_filtered_batch) ---- */
static void finalize_filter(napi_env env, void *data, void *hint) {
  (void)env; (void)hint;
  bbq_filter **box = (bbq_filter **)data;
  if (*box) bbq_filter_destroy(*box);
  free(box);
}

/* filterCreate(index handle, Uint8Array mask [size()] (non-zero = accepted) | Int32Array rows) -> {handle, count} */
static napi_value FilterCreate(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  bool is = false;
  napi_typedarray_type t;
  napi_value ab;
  size_t len, off;
  void *data;
  if (napi_is_typedarray(env, a[1], &is) != napi_ok || !is || napi_get_typedarray_info(env, a[1], &t, &len, &data, &ab, &off) != napi_ok ||
      (t != napi_uint8_array && t != napi_int32_array)) {
    napi_throw_type_error(env, NULL, "bbq_napi: a filter is a Uint8Array mask or an Int32Array of rows");
    return NULL;
  }
  bbq_filter **box = (bbq_filter **)calloc(1, sizeof *box);
  if (!box) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc;
  if (t == napi_int32_array) {
    rc = bbq_filter_create_rows(ix, (const int32_t *)data, (int64_t)len, box);
  } else {
    const int64_t n = bbq_index_size(ix), nw = (n + 63) / 64;
    if ((int64_t)len != n) { free(box); napi_throw_range_error(env, NULL, "bbq_napi: a filter mask has one entry per row of the index"); return NULL; }
    uint64_t *words = (uint64_t *)calloc((size_t)nw + 1, sizeof *words);
    if (!words) { free(box); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
    for (int64_t r = 0; r < n; ++r)
      if (((const uint8_t *)data)[r]) words[r >> 6] |= 1ull << (r & 63);
    rc = bbq_filter_create(ix, words, nw, box);
    free(words);
  }
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext, o, cnt;
  if (napi_create_external(env, box, finalize_filter, NULL, &ext) != napi_ok) { bbq_filter_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  NAPI_CALL(env, napi_create_object(env, &o));
  NAPI_CALL(env, napi_create_double(env, (double)bbq_filter_count(*box), &cnt));
  set_prop(env, o, "handle", ext); set_prop(env, o, "count", cnt);
  return o;
}

/* filterDestroy(handle) */
static napi_value FilterDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  void *p = NULL;
  if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
    bbq_filter **box = (bbq_filter **)p;
    if (*box) { bbq_filter_destroy(*box); *box = NULL; }
  }
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* the filter behind a handle of filterCreate, or NULL with an exception pending */
static const bbq_filter *unbox_filter(napi_env env, napi_value v, const char *who) {
  void *fp = NULL;
  if (napi_get_value_external(env, v, &fp) != napi_ok || !fp || !*(bbq_filter **)fp) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: the filter is null", who);
    napi_throw_error(env, "BBQ1", msg);
    return NULL;
  }
  return *(bbq_filter **)fp;
}

/* indexCompact(index handle, filter handle) -> rows afterwards: the index becomes the index over the accepted rows, on the device
 * (bbq_index_compact) */
static napi_value IndexCompact(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  const bbq_filter *flt = unbox_filter(env, a[1], "bbq_index_compact");
  if (!flt) return NULL;
  int rc = bbq_index_compact(ix, flt);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value r;
  NAPI_CALL(env, napi_create_double(env, (double)bbq_index_size(ix), &r));
  return r;
}

/* searchFilteredBatch(index handle, filter handle, nq, qquant, qcorr, queryBits, sim, k) -> as searchBatch, rows strided by min(k, |A|) */
static napi_value SearchFilteredBatch(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *fp = NULL;
  if (napi_get_value_external(env, a[1], &fp) != napi_ok || !fp || !*(bbq_filter **)fp) {
    napi_throw_error(env, "BBQ1", "bbq_search_filtered_batch: the filter is null");
    return NULL;
  }
  const bbq_filter *flt = *(bbq_filter **)fp;
  void *qq, *qc; size_t ql, cl;
  int64_t nq, qb, sim, k;
  if (!get_i64(env, a[2], &nq) || !get_typed(env, a[3], napi_uint8_array, &qq, &ql) || !get_typed(env, a[4], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[5], &qb) || !get_i64(env, a[6], &sim) || !get_i64(env, a[7], &k)) return NULL;
  if (nq < 0 || ql != (size_t)nq * (size_t)bbq_index_dimension(ix) || cl != (size_t)nq * 4) {
    napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL;
  }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  int64_t keff = k < bbq_filter_count(flt) ? k : bbq_filter_count(flt);
  void *oi, *os, *on;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)(nq * keff), 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)(nq * keff), 4, &os);
  napi_value tn = new_typed(env, napi_float64_array, (size_t)nq, 8, &on);
  if (!ti || !ts || !tn) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t *cnt = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
  if (!cnt) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_search_filtered_batch(ix, flt, (int32_t)nq, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, (int32_t *)oi, (float *)os, cnt);
  if (rc != BBQ_OK) { free(cnt); return throw_bbq(env, rc); }
  for (int64_t i = 0; i < nq; ++i) ((double *)on)[i] = (double)cnt[i];
  free(cnt);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts); set_prop(env, o, "counts", tn);
  napi_value kv; napi_create_double(env, (double)keff, &kv); set_prop(env, o, "stride", kv);
  return o;
}

/* searchRawBatch(handle, nq, flat Float32Array[nq*dim] raw queries, centroid Float32Array[dim], sim, queryBits, lambda, iters, threads, k)
 *   -> {indices, scores, counts, stride}   (bbq_search_raw_batch: quantization on host threads pipelined with the sweeps) */
static napi_value SearchRawBatch(napi_env env, napi_callback_info info) {
  napi_value a[10];
  if (!get_args(env, info, 10, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *q, *cen; size_t ql, cl;
  int64_t nq, sim, qb, iters, threads, k; double lambda;
  if (!get_i64(env, a[1], &nq) || !get_typed(env, a[2], napi_float32_array, &q, &ql) || !get_typed(env, a[3], napi_float32_array, &cen, &cl) ||
      !get_i64(env, a[4], &sim) || !get_i64(env, a[5], &qb) || !get_f64(env, a[6], &lambda) || !get_i64(env, a[7], &iters) ||
      !get_i64(env, a[8], &threads) || !get_i64(env, a[9], &k)) return NULL;
  if (nq < 0 || cl != (size_t)bbq_index_dimension(ix) || ql != (size_t)nq * cl) {
    napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL;
  }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  int64_t keff = k < bbq_index_size(ix) ? k : bbq_index_size(ix);
  void *oi, *os, *on;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)(nq * keff), 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)(nq * keff), 4, &os);
  napi_value tn = new_typed(env, napi_float64_array, (size_t)nq, 8, &on);
  if (!ti || !ts || !tn) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t *cnt = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
  int rc = bbq_search_raw_batch(ix, (int32_t)nq, (const float *)q, (const float *)cen, (int32_t)sim, (int32_t)qb, lambda, (int32_t)iters,
                                (int32_t)threads, keff, (int32_t *)oi, (float *)os, cnt, NULL, NULL, NULL);
  if (rc != BBQ_OK) { free(cnt); return throw_bbq(env, rc); }
  for (int64_t i = 0; i < nq; ++i) ((double *)on)[i] = (double)cnt[i];
  free(cnt);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts); set_prop(env, o, "counts", tn);
  napi_value kv; napi_create_double(env, (double)keff, &kv); set_prop(env, o, "stride", kv);
  return o;
}

/* searchRawInto(handle, query Float32Array[dim] raw, centroid Float32Array[dim], sim, queryBits, lambda, iters, k, outIndices Int32Array[>= k],
 *               outScores Float32Array[>= k]) -> count
 * The reference's own call shape - ONE synchronous searchNearestNeighbors (src/binaryQuantizationFormat.ts:308-412) - without a typed
 * array or an object created per call: the caller owns and reuses the output arrays.  (Every ArrayBuffer the batch form creates counts
 * as external memory; their collection was the 0.8 ms tail of a 0.2 ms call.) */
static napi_value SearchRawInto(napi_env env, napi_callback_info info) {
  napi_value a[10];
  if (!get_args(env, info, 10, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *q, *cen, *oi, *os; size_t ql, cl, il, sl;
  int64_t sim, qb, iters, k; double lambda;
  if (!get_typed(env, a[1], napi_float32_array, &q, &ql) || !get_typed(env, a[2], napi_float32_array, &cen, &cl) ||
      !get_i64(env, a[3], &sim) || !get_i64(env, a[4], &qb) || !get_f64(env, a[5], &lambda) || !get_i64(env, a[6], &iters) ||
      !get_i64(env, a[7], &k) || !get_typed(env, a[8], napi_int32_array, &oi, &il) || !get_typed(env, a[9], napi_float32_array, &os, &sl)) return NULL;
  if (cl != (size_t)bbq_index_dimension(ix) || ql != cl) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  int64_t keff = k < bbq_index_size(ix) ? k : bbq_index_size(ix);
  if (il < (size_t)keff || sl < (size_t)keff) { napi_throw_error(env, NULL, "bbq_napi: output arrays shorter than k"); return NULL; }
  int64_t cnt[2] = {0, 0};
  int rc = bbq_search_raw_batch(ix, 1, (const float *)q, (const float *)cen, (int32_t)sim, (int32_t)qb, lambda, (int32_t)iters, 1, keff,
                                (int32_t *)oi, (float *)os, cnt, NULL, NULL, NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value n;
  NAPI_CALL(env, napi_create_double(env, (double)cnt[0], &n));
  return n;
}

/* scoreRows(handle, qquant, qcorr, queryBits, sim, rowBegin, rowCount) -> {qcDist Int32Array, score64 Float64Array, score32 Float32Array} */
static napi_value ScoreRows(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *qq, *qc; size_t ql, cl;
  int64_t qb, sim, rb, rc_;
  if (!get_typed(env, a[1], napi_uint8_array, &qq, &ql) || !get_typed(env, a[2], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[3], &qb) || !get_i64(env, a[4], &sim) || !get_i64(env, a[5], &rb) || !get_i64(env, a[6], &rc_)) return NULL;
  if (ql != (size_t)bbq_index_dimension(ix) || cl != 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (rc_ < 0) rc_ = 0;
  void *od, *o64, *o32;
  napi_value td = new_typed(env, napi_int32_array, (size_t)rc_, 4, &od);
  napi_value t64 = new_typed(env, napi_float64_array, (size_t)rc_, 8, &o64);
  napi_value t32 = new_typed(env, napi_float32_array, (size_t)rc_, 4, &o32);
  if (!td || !t64 || !t32) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_score_rows(ix, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, rb, rc_, (int32_t *)od, (double *)o64, (float *)o32);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "qcDist", td); set_prop(env, o, "score64", t64); set_prop(env, o, "score32", t32);
  return o;
}

/* scoreOrds(handle, qquant, qcorr, queryBits, sim, ords Int32Array) -> {qcDist Int32Array, score64 Float64Array, score32 Float32Array}, indexed like ords
 * (bbq_score_ords: any order, duplicates allowed; an ord that names no row throws the reference's message) */
static napi_value ScoreOrds(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (!get_args(env, info, 6, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *qq, *qc, *ords; size_t ql, cl, n;
  int64_t qb, sim;
  if (!get_typed(env, a[1], napi_uint8_array, &qq, &ql) || !get_typed(env, a[2], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[3], &qb) || !get_i64(env, a[4], &sim) || !get_typed(env, a[5], napi_int32_array, &ords, &n)) return NULL;
  if (ql != (size_t)bbq_index_dimension(ix) || cl != 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  void *od, *o64, *o32;
  napi_value td = new_typed(env, napi_int32_array, n, 4, &od);
  napi_value t64 = new_typed(env, napi_float64_array, n, 8, &o64);
  napi_value t32 = new_typed(env, napi_float32_array, n, 4, &o32);
  if (!td || !t64 || !t32) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_score_ords(ix, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, (const int32_t *)ords, (int64_t)n, (int32_t *)od, (double *)o64, (float *)o32);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "qcDist", td); set_prop(env, o, "score64", t64); set_prop(env, o, "score32", t32);
  return o;
}

/* searchOrds(handle, qquant, qcorr, queryBits, sim, k, ords Int32Array) -> {indices Int32Array, scores Float32Array} of min(k, ords.length) entries:
 * the reference's loop over `ords` in the order given (bbq_search_ords_batch with one query) */
static napi_value SearchOrds(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *qq, *qc, *ords; size_t ql, cl, n;
  int64_t qb, sim, k;
  if (!get_typed(env, a[1], napi_uint8_array, &qq, &ql) || !get_typed(env, a[2], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[3], &qb) || !get_i64(env, a[4], &sim) || !get_i64(env, a[5], &k) || !get_typed(env, a[6], napi_int32_array, &ords, &n)) return NULL;
  if (ql != (size_t)bbq_index_dimension(ix) || cl != 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  const int64_t keff = k < (int64_t)n ? k : (int64_t)n;
  const int64_t offsets[2] = {0, (int64_t)n};
  int64_t cnt = 0;
  int32_t *idx = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  float *sc = (float *)malloc(((size_t)keff + 1) * sizeof(float));
  if (!idx || !sc) { free(idx); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_search_ords_batch(ix, 1, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, offsets, (const int32_t *)ords, idx, sc, &cnt);
  if (rc != BBQ_OK) { free(idx); free(sc); return throw_bbq(env, rc); }
  void *oi, *os;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)cnt, 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)cnt, 4, &os);
  if (!ti || !ts) { free(idx); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  if (cnt > 0) { memcpy(oi, idx, (size_t)cnt * 4); memcpy(os, sc, (size_t)cnt * 4); }
  free(idx); free(sc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts);
  return o;
}

/* what searchSpans and searchSpansFiltered share: a = qquant, qcorr, queryBits, sim, k, spans; flt = the row filter, or NULL: every row */
static napi_value search_spans(napi_env env, bbq_index *ix, const bbq_filter *flt, const napi_value *a) {
  void *qq, *qc, *sp; size_t ql, cl, n2;
  int64_t qb, sim, k;
  if (!get_typed(env, a[0], napi_uint8_array, &qq, &ql) || !get_typed(env, a[1], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[2], &qb) || !get_i64(env, a[3], &sim) || !get_i64(env, a[4], &k) || !get_typed(env, a[5], napi_float64_array, &sp, &n2)) return NULL;
  if (ql != (size_t)bbq_index_dimension(ix) || cl != 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  if (n2 % 2 != 0) { napi_throw_range_error(env, NULL, "bbq_napi: spans are pairs of begin and end"); return NULL; }
  const int64_t size = bbq_index_size(ix);
  const int64_t keff = k < size ? k : size;   /* no answer is longer than the index */
  int64_t *s64 = (int64_t *)malloc((n2 + 1) * sizeof(int64_t));
  int32_t *idx = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  float *sc = (float *)malloc(((size_t)keff + 1) * sizeof(float));
  if (!s64 || !idx || !sc) { free(s64); free(idx); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  for (size_t i = 0; i < n2; ++i) {
    const double v = ((const double *)sp)[i];
    if (!(v >= -9007199254740992.0 && v <= 9007199254740992.0) || v != (double)(int64_t)v) {
      free(s64); free(idx); free(sc);
      napi_throw_range_error(env, NULL, "bbq_napi: a span's begin and end are integers");
      return NULL;
    }
    s64[i] = (int64_t)v;
  }
  const int64_t offsets[2] = {0, (int64_t)(n2 / 2)};
  int64_t cnt = 0;
  uint8_t status = 0;
  int rc = flt ? bbq_search_spans_filtered_batch(ix, flt, 1, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, offsets, s64, idx, sc, &cnt, &status)
               : bbq_search_spans_batch(ix, 1, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, offsets, s64, idx, sc, &cnt, &status);
  free(s64);
  if (rc != BBQ_OK) { free(idx); free(sc); return throw_bbq(env, rc); }
  void *oi, *os;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)cnt, 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)cnt, 4, &os);
  if (!ti || !ts) { free(idx); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  if (cnt > 0) { memcpy(oi, idx, (size_t)cnt * 4); memcpy(os, sc, (size_t)cnt * 4); }
  free(idx); free(sc);
  napi_value o, st;
  NAPI_CALL(env, napi_create_object(env, &o));
  NAPI_CALL(env, napi_create_int32(env, (int32_t)status, &st));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts); set_prop(env, o, "status", st);
  return o;
}

/* searchSpans(handle, qquant, qcorr, queryBits, sim, k, spans Float64Array [2 m] = begin, end (exclusive) of each span) ->
 * {indices Int32Array, scores Float32Array, status}: the reference's loop over the rows of the spans, ascending (bbq_search_spans_batch
 * with one query); status 0: the device selected the answer, 1: the host replayed the heap */
static napi_value SearchSpans(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  return search_spans(env, ix, NULL, a + 1);
}

/* searchSpansFiltered(handle, filter handle, qquant, qcorr, queryBits, sim, k, spans) -> as searchSpans, over the rows of the spans that
 * the filter accepts (bbq_search_spans_filtered_batch with one query) */
static napi_value SearchSpansFiltered(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  const bbq_filter *flt = unbox_filter(env, a[1], "bbq_search_spans_filtered_batch");
  if (!flt) return NULL;
  return search_spans(env, ix, flt, a + 2);
}

/* ---- grouped search (bbq_groups_*, bbq_search_grouped_batch) ---- */
static void finalize_groups(napi_env env, void *data, void *hint) {
  (void)env; (void)hint;
  bbq_groups **box = (bbq_groups **)data;
  if (*box) bbq_groups_destroy(*box);
  free(box);
}

/* groupsCreate(index handle, offsets Float64Array [groups + 1], filter handle | null) -> {handle, count, live} */
static napi_value GroupsCreate(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!get_args(env, info, 3, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *op; size_t n;
  if (!get_typed(env, a[1], napi_float64_array, &op, &n)) return NULL;
  const bbq_filter *flt = NULL;
  napi_valuetype vt;
  NAPI_CALL(env, napi_typeof(env, a[2], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    flt = unbox_filter(env, a[2], "bbq_groups_create");
    if (!flt) return NULL;
  }
  if (n < 1) { napi_throw_range_error(env, NULL, "bbq_napi: group offsets hold one entry per group and one more"); return NULL; }
  int64_t *off = (int64_t *)malloc(n * sizeof(int64_t));
  bbq_groups **box = (bbq_groups **)calloc(1, sizeof *box);
  if (!off || !box) { free(off); free(box); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  for (size_t i = 0; i < n; ++i) {
    const double v = ((const double *)op)[i];
    if (!(v >= -9007199254740992.0 && v <= 9007199254740992.0) || v != (double)(int64_t)v) {
      free(off); free(box);
      napi_throw_range_error(env, NULL, "bbq_napi: group offsets are integers");
      return NULL;
    }
    off[i] = (int64_t)v;
  }
  int rc = bbq_groups_create(ix, off, (int64_t)n - 1, flt, box);
  free(off);
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext, o, cnt, live;
  if (napi_create_external(env, box, finalize_groups, NULL, &ext) != napi_ok) { bbq_groups_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  NAPI_CALL(env, napi_create_object(env, &o));
  NAPI_CALL(env, napi_create_double(env, (double)bbq_groups_count(*box), &cnt));
  NAPI_CALL(env, napi_create_double(env, (double)bbq_groups_live(*box), &live));
  set_prop(env, o, "handle", ext); set_prop(env, o, "count", cnt); set_prop(env, o, "live", live);
  return o;
}

/* groupsDestroy(handle) */
static napi_value GroupsDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  void *p = NULL;
  if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
    bbq_groups **box = (bbq_groups **)p;
    if (*box) { bbq_groups_destroy(*box); *box = NULL; }
  }
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* searchGrouped(handle, groups handle, qquant, qcorr, queryBits, sim, k) -> {indices Int32Array, scores Float32Array, groups Int32Array,
 * status}: the k best groups, each through its best accepted row (bbq_search_grouped_batch with one query); status 0: the device
 * selected the answer, 1: the host replayed the heap */
static napi_value SearchGrouped(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *gp = NULL;
  if (napi_get_value_external(env, a[1], &gp) != napi_ok || !gp || !*(bbq_groups **)gp) {
    napi_throw_error(env, "BBQ1", "bbq_search_grouped_batch: the group set is null");
    return NULL;
  }
  const bbq_groups *grp = *(bbq_groups **)gp;
  void *qq, *qc; size_t ql, cl;
  int64_t qb, sim, k;
  if (!get_typed(env, a[2], napi_uint8_array, &qq, &ql) || !get_typed(env, a[3], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[4], &qb) || !get_i64(env, a[5], &sim) || !get_i64(env, a[6], &k)) return NULL;
  if (ql != (size_t)bbq_index_dimension(ix) || cl != 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  const int64_t live = bbq_groups_live(grp);
  const int64_t keff = k < live ? k : live;   /* no answer is longer than the live groups */
  int32_t *idx = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  int32_t *og = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  float *sc = (float *)malloc(((size_t)keff + 1) * sizeof(float));
  if (!idx || !og || !sc) { free(idx); free(og); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t cnt = 0;
  uint8_t status = 0;
  int rc = bbq_search_grouped_batch(ix, grp, 1, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, idx, og, sc, &cnt, &status);
  if (rc != BBQ_OK) { free(idx); free(og); free(sc); return throw_bbq(env, rc); }
  void *oi, *os, *ogp;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)cnt, 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)cnt, 4, &os);
  napi_value tg = new_typed(env, napi_int32_array, (size_t)cnt, 4, &ogp);
  if (!ti || !ts || !tg) { free(idx); free(og); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  if (cnt > 0) { memcpy(oi, idx, (size_t)cnt * 4); memcpy(os, sc, (size_t)cnt * 4); memcpy(ogp, og, (size_t)cnt * 4); }
  free(idx); free(og); free(sc);
  napi_value o, st;
  NAPI_CALL(env, napi_create_object(env, &o));
  NAPI_CALL(env, napi_create_int32(env, (int32_t)status, &st));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts); set_prop(env, o, "groups", tg); set_prop(env, o, "status", st);
  return o;
}

/* searchMaxSim(handle, groups handle, qquant [T * dim], qcorr [T * 4], queryBits, sim, k) -> {groups Int32Array, scores Float32Array,
 * status}: the k best groups for ONE query of T >= 1 token vectors, each group scoring the ordered sum of its best accepted rows' scores
 * (bbq_search_maxsim_batch with one query); status 0: the device selected the answer, 1: the host replayed the heap */
static napi_value SearchMaxSim(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  void *gp = NULL;
  if (napi_get_value_external(env, a[1], &gp) != napi_ok || !gp || !*(bbq_groups **)gp) {
    napi_throw_error(env, "BBQ1", "bbq_search_maxsim_batch: the group set is null");
    return NULL;
  }
  const bbq_groups *grp = *(bbq_groups **)gp;
  void *qq, *qc; size_t ql, cl;
  int64_t qb, sim, k;
  if (!get_typed(env, a[2], napi_uint8_array, &qq, &ql) || !get_typed(env, a[3], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[4], &qb) || !get_i64(env, a[5], &sim) || !get_i64(env, a[6], &k)) return NULL;
  const size_t dim = (size_t)bbq_index_dimension(ix);
  if (dim == 0 || ql == 0 || ql % dim != 0 || cl != ql / dim * 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  const int64_t live = bbq_groups_live(grp);
  const int64_t keff = k < live ? k : live;   /* no answer is longer than the live groups */
  const int64_t voff[2] = {0, (int64_t)(ql / dim)};
  int32_t *og = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  float *sc = (float *)malloc(((size_t)keff + 1) * sizeof(float));
  if (!og || !sc) { free(og); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t cnt = 0;
  uint8_t status = 0;
  int rc = bbq_search_maxsim_batch(ix, grp, 1, voff, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, og, sc, &cnt, &status);
  if (rc != BBQ_OK) { free(og); free(sc); return throw_bbq(env, rc); }
  void *os, *ogp;
  napi_value ts = new_typed(env, napi_float32_array, (size_t)cnt, 4, &os);
  napi_value tg = new_typed(env, napi_int32_array, (size_t)cnt, 4, &ogp);
  if (!ts || !tg) { free(og); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  if (cnt > 0) { memcpy(os, sc, (size_t)cnt * 4); memcpy(ogp, og, (size_t)cnt * 4); }
  free(og); free(sc);
  napi_value o, st;
  NAPI_CALL(env, napi_create_object(env, &o));
  NAPI_CALL(env, napi_create_int32(env, (int32_t)status, &st));
  set_prop(env, o, "groups", tg); set_prop(env, o, "scores", ts); set_prop(env, o, "status", st);
  return o;
}

/* the arguments scoreMaxSimGroups and searchMaxSimGroups share: (handle, groups handle, qquant [T * dim], qcorr [T * 4], queryBits, sim, ...) */
static int maxsim_groups_args(napi_env env, napi_value *a, const char *fn, bbq_index **ix, const bbq_groups **grp, void **qq, void **qc, int64_t *qb,
                              int64_t *sim, int64_t *n_tok) {
  *ix = unbox(env, a[0]);
  if (!*ix) return 0;
  void *gp = NULL;
  if (napi_get_value_external(env, a[1], &gp) != napi_ok || !gp || !*(bbq_groups **)gp) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: the group set is null", fn);
    napi_throw_error(env, "BBQ1", msg);
    return 0;
  }
  *grp = *(bbq_groups **)gp;
  size_t ql, cl;
  if (!get_typed(env, a[2], napi_uint8_array, qq, &ql) || !get_typed(env, a[3], napi_float64_array, qc, &cl) || !get_i64(env, a[4], qb) ||
      !get_i64(env, a[5], sim)) return 0;
  const size_t dim = (size_t)bbq_index_dimension(*ix);
  if (dim == 0 || ql == 0 || ql % dim != 0 || cl != ql / dim * 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return 0; }
  *n_tok = (int64_t)(ql / dim);
  return 1;
}

/* scoreMaxSimGroups(handle, groups handle, qquant, qcorr, queryBits, sim, candidates Int32Array) -> Float32Array: the MaxSim score of every
 * candidate group, in list order, for ONE query of T >= 1 token vectors (bbq_score_maxsim_groups_batch with one query) */
static napi_value ScoreMaxSimGroups(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix; const bbq_groups *grp; void *qq, *qc, *cg; int64_t qb, sim, n_tok; size_t nc;
  if (!maxsim_groups_args(env, a, "bbq_score_maxsim_groups_batch", &ix, &grp, &qq, &qc, &qb, &sim, &n_tok)) return NULL;
  if (!get_typed(env, a[6], napi_int32_array, &cg, &nc)) return NULL;
  const int64_t voff[2] = {0, n_tok}, coff[2] = {0, (int64_t)nc};
  void *os;
  napi_value ts = new_typed(env, napi_float32_array, nc, 4, &os);
  if (!ts) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_score_maxsim_groups_batch(ix, grp, 1, voff, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, coff, (const int32_t *)cg,
                                         (float *)os);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  return ts;
}

/* searchMaxSimGroups(handle, groups handle, qquant, qcorr, queryBits, sim, k, candidates Int32Array) -> {groups Int32Array, scores
 * Float32Array}: the k best of the candidates, visited in list order (bbq_search_maxsim_groups_batch with one query) */
static napi_value SearchMaxSimGroups(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  bbq_index *ix; const bbq_groups *grp; void *qq, *qc, *cg; int64_t qb, sim, n_tok, k; size_t nc;
  if (!maxsim_groups_args(env, a, "bbq_search_maxsim_groups_batch", &ix, &grp, &qq, &qc, &qb, &sim, &n_tok)) return NULL;
  if (!get_i64(env, a[6], &k) || !get_typed(env, a[7], napi_int32_array, &cg, &nc)) return NULL;
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  const int64_t keff = k < (int64_t)nc ? k : (int64_t)nc;   /* no answer is longer than the list */
  const int64_t voff[2] = {0, n_tok}, coff[2] = {0, (int64_t)nc};
  int32_t *og = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  float *sc = (float *)malloc(((size_t)keff + 1) * sizeof(float));
  if (!og || !sc) { free(og); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t cnt = 0;
  int rc = bbq_search_maxsim_groups_batch(ix, grp, 1, voff, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff, coff,
                                          (const int32_t *)cg, og, sc, &cnt);
  if (rc != BBQ_OK) { free(og); free(sc); return throw_bbq(env, rc); }
  void *os, *ogp;
  napi_value ts = new_typed(env, napi_float32_array, (size_t)cnt, 4, &os);
  napi_value tg = new_typed(env, napi_int32_array, (size_t)cnt, 4, &ogp);
  if (!ts || !tg) { free(og); free(sc); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  if (cnt > 0) { memcpy(os, sc, (size_t)cnt * 4); memcpy(ogp, og, (size_t)cnt * 4); }
  free(og); free(sc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "groups", tg); set_prop(env, o, "scores", ts);
  return o;
}

/* searchRange(handle, filter handle | null, qquant, qcorr, queryBits, sim, threshold) ->{indices Int32Array, scores Float32Array}: every row (of
 * the filter, if one is given) whose f32 score is >= threshold, ascending by ord (bbq_count_range_batch, then bbq_search_range_batch with
 * exactly that room).  A NaN threshold throws. */
static napi_value SearchRange(napi_env env, napi_callback_info info) {
  napi_value a[7];
  if (!get_args(env, info, 7, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  const bbq_filter *flt = NULL;
  napi_valuetype vt;
  NAPI_CALL(env, napi_typeof(env, a[1], &vt));
  if (vt != napi_null && vt != napi_undefined) {
    flt = unbox_filter(env, a[1], "bbq_search_range_batch");
    if (!flt) return NULL;
  }
  void *qq, *qc; size_t ql, cl;
  int64_t qb, sim; double t;
  if (!get_typed(env, a[2], napi_uint8_array, &qq, &ql) || !get_typed(env, a[3], napi_float64_array, &qc, &cl) ||
      !get_i64(env, a[4], &qb) || !get_i64(env, a[5], &sim) || !get_f64(env, a[6], &t)) return NULL;
  if (ql != (size_t)bbq_index_dimension(ix) || cl != 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  const float th = (float)t;
  int64_t total = 0, offsets[2] = {0, 0};
  int rc = bbq_count_range_batch(ix, flt, 1, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, &th, &total);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  void *oi, *os;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)total, 4, &oi);
  napi_value ts = new_typed(env, napi_float32_array, (size_t)total, 4, &os);
  if (!ti || !ts) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  rc = bbq_search_range_batch(ix, flt, 1, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, &th, total, offsets,
                              total ? (int32_t *)oi : NULL, total ? (float *)os : NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "scores", ts);
  return o;
}

/* setOption(handle, name, value) */
static napi_value SetOption(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!get_args(env, info, 3, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  char name[64]; size_t nl; int64_t v;
  NAPI_CALL(env, napi_get_value_string_utf8(env, a[1], name, sizeof name, &nl));
  if (!get_i64(env, a[2], &v)) return NULL;
  int rc = bbq_set_option(ix, name, v);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* stats(handle) -> {lastScanMs, lastScanBytes, candidates, denseFallbacks} */
static napi_value Stats(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  bbq_stats st;
  int rc = bbq_get_stats(ix, &st);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o, v;
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_create_double(env, st.last_scan_ms, &v); set_prop(env, o, "lastScanMs", v);
  napi_create_double(env, (double)st.last_scan_bytes, &v); set_prop(env, o, "lastScanBytes", v);
  napi_create_double(env, (double)st.candidates, &v); set_prop(env, o, "candidates", v);
  napi_create_double(env, (double)st.dense_fallbacks, &v); set_prop(env, o, "denseFallbacks", v);
  napi_create_double(env, (double)st.host_replays, &v); set_prop(env, o, "hostReplays", v);
  napi_create_double(env, (double)st.resident_bytes, &v); set_prop(env, o, "residentBytes", v);
  napi_create_double(env, (double)bbq_index_shards(ix), &v); set_prop(env, o, "shards", v);
  napi_create_double(env, (double)bbq_index_bytes_per_row(ix), &v); set_prop(env, o, "bytesPerRow", v);
  return o;
}

/* ---- oversample + exact rerank (bbq_vectors_*, bbq_rerank_scores, bbq_search_rerank_batch) */
static void finalize_vectors(napi_env env, void *data, void *hint) {
  (void)env; (void)hint;
  bbq_vectors **box = (bbq_vectors **)data;
  if (*box) bbq_vectors_destroy(*box);
  free(box);
}

static bbq_vectors *unbox_vectors(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || !*(bbq_vectors **)p) {
    napi_throw_error(env, NULL, "向量不能为空");
    return NULL;
  }
  return *(bbq_vectors **)p;
}

/* vectorsCreate(flat Float32Array, n, dim, device) -> external */
static napi_value VectorsCreate(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!get_args(env, info, 4, a)) return NULL;
  void *vec; size_t vlen;
  int64_t n, dim, dev;
  if (!get_typed(env, a[0], napi_float32_array, &vec, &vlen) || !get_i64(env, a[1], &n) || !get_i64(env, a[2], &dim) ||
      !get_i64(env, a[3], &dev)) return NULL;
  if (n < 0 || dim <= 0 || (size_t)(n * dim) != vlen) { napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the array"); return NULL; }
  bbq_vectors **box = (bbq_vectors **)calloc(1, sizeof *box);
  int rc = bbq_vectors_create((const float *)vec, n, (int32_t)dim, (int32_t)dev, box);
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext;
  if (napi_create_external(env, box, finalize_vectors, NULL, &ext) != napi_ok) { bbq_vectors_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  return ext;
}

/* vectorsAppend(handle, flat Float32Array, n, dim): the fp32 rows of an appended block (bbq_vectors_append) */
static napi_value VectorsAppend(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!get_args(env, info, 4, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  void *vec; size_t vlen;
  int64_t n, dim;
  if (!get_typed(env, a[1], napi_float32_array, &vec, &vlen) || !get_i64(env, a[2], &n) || !get_i64(env, a[3], &dim)) return NULL;
  if (n < 0 || dim != bbq_vectors_dimension(v) || (size_t)(n * dim) != vlen) { napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the array or the vectors"); return NULL; }
  int rc = bbq_vectors_append(v, (const float *)vec, n);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* vectorsUpdate(handle, ords Int32Array[n], flat Float32Array, n, dim): the fp32 rows of an update block (bbq_vectors_update) */
static napi_value VectorsUpdate(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!get_args(env, info, 5, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  void *ords, *vec; size_t ol, vlen;
  int64_t n, dim;
  if (!get_typed(env, a[1], napi_int32_array, &ords, &ol) || !get_typed(env, a[2], napi_float32_array, &vec, &vlen) || !get_i64(env, a[3], &n) ||
      !get_i64(env, a[4], &dim)) return NULL;
  if (n < 0 || dim != bbq_vectors_dimension(v) || (size_t)(n * dim) != vlen || ol != (size_t)n) {
    napi_throw_range_error(env, NULL, "bbq_napi: n*dim does not match the arrays or the vectors"); return NULL;
  }
  int rc = bbq_vectors_update(v, (const int32_t *)ords, (const float *)vec, n);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* vectorsCompact(vectors handle, filter handle) -> rows afterwards: the fp32 rows follow a compaction of the index (bbq_vectors_compact) */
static napi_value VectorsCompact(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  const bbq_filter *flt = unbox_filter(env, a[1], "bbq_vectors_compact");
  if (!flt) return NULL;
  int rc = bbq_vectors_compact(v, flt);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value r;
  NAPI_CALL(env, napi_create_double(env, (double)bbq_vectors_size(v), &r));
  return r;
}

/* vectorsDestroy(handle) */
static napi_value VectorsDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  void *p = NULL;
  if (napi_get_value_external(env, a[0], &p) == napi_ok && p) {
    bbq_vectors **box = (bbq_vectors **)p;
    if (*box) { bbq_vectors_destroy(*box); *box = NULL; }
  }
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* rerankScores(vectors, nq, queries Float32Array[nq*dim], offsets Float64Array[nq+1], rows Int32Array, trueSim) -> Float64Array */
static napi_value RerankScores(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (!get_args(env, info, 6, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  void *q, *off, *rows; size_t ql, ol, rl;
  int64_t nq, sim;
  if (!get_i64(env, a[1], &nq) || !get_typed(env, a[2], napi_float32_array, &q, &ql) || !get_typed(env, a[3], napi_float64_array, &off, &ol) ||
      !get_typed(env, a[4], napi_int32_array, &rows, &rl) || !get_i64(env, a[5], &sim)) return NULL;
  if (nq < 0 || ql != (size_t)nq * (size_t)bbq_vectors_dimension(v)) { napi_throw_error(env, "BBQ6", "向量维度不匹配"); return NULL; }
  if (ol != (size_t)nq + 1) { napi_throw_range_error(env, NULL, "bbq_napi: offsets must have nq+1 entries"); return NULL; }
  int64_t *o64 = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
  for (int64_t i = 0; i <= nq; ++i) o64[i] = (int64_t)((double *)off)[i];
  if (o64[nq] < 0 || (size_t)o64[nq] != rl) { free(o64); napi_throw_range_error(env, NULL, "bbq_napi: offsets do not match rows"); return NULL; }
  void *out;
  napi_value t = new_typed(env, napi_float64_array, rl, 8, &out);
  if (!t) { free(o64); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_rerank_scores(v, (int32_t)nq, (const float *)q, o64, (const int32_t *)rows, (int32_t)sim, (double *)out);
  free(o64);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  return t;
}

/* vectorsSearchBatch(vectors, filter handle | null, nq, queries Float32Array[nq*dim], trueSim, k) -> {indices Int32Array[nq*k], trueScores
 * Float64Array[nq*k], counts Float64Array[nq], stride}: the exact top-k of every raw query over the resident rows (bbq_vectors_search_batch) */
static napi_value VectorsSearchBatch(napi_env env, napi_callback_info info) {
  napi_value a[6];
  if (!get_args(env, info, 6, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  const bbq_filter *flt = NULL;
  napi_valuetype ft;
  NAPI_CALL(env, napi_typeof(env, a[1], &ft));
  if (ft != napi_null && ft != napi_undefined) {
    flt = unbox_filter(env, a[1], "bbq_vectors_search_batch");
    if (!flt) return NULL;
  }
  void *q; size_t ql;
  int64_t nq, sim, k;
  if (!get_i64(env, a[2], &nq) || !get_typed(env, a[3], napi_float32_array, &q, &ql) || !get_i64(env, a[4], &sim) || !get_i64(env, a[5], &k)) return NULL;
  if (nq < 0 || nq > 0x7fffffff || ql != (size_t)nq * (size_t)bbq_vectors_dimension(v)) { napi_throw_error(env, "BBQ6", "向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  if (k > 4096) k = 4097;  /* the same answer - min(k, accepted rows) beyond 4096 is refused either way - from arrays that stay small */
  void *oi, *ot, *on;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)(nq * k), 4, &oi);
  napi_value tt = new_typed(env, napi_float64_array, (size_t)(nq * k), 8, &ot);
  napi_value tn = new_typed(env, napi_float64_array, (size_t)nq, 8, &on);
  if (!ti || !tt || !tn) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t *cnt = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
  if (!cnt) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_vectors_search_batch(v, flt, (int32_t)nq, (const float *)q, (int32_t)sim, k, (int32_t *)oi, (double *)ot, cnt);
  if (rc != BBQ_OK) { free(cnt); return throw_bbq(env, rc); }
  for (int64_t i = 0; i < nq; ++i) ((double *)on)[i] = (double)cnt[i];
  free(cnt);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "trueScores", tt); set_prop(env, o, "counts", tn);
  napi_value kv; napi_create_double(env, (double)k, &kv); set_prop(env, o, "stride", kv);
  return o;
}

/* vectorsSetOption(vectors, name, value) (bbq_vectors_set_option) */
static napi_value VectorsSetOption(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!get_args(env, info, 3, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  char name[64]; size_t nl = 0;
  int64_t value;
  if (napi_get_value_string_utf8(env, a[1], name, sizeof name, &nl) != napi_ok) { napi_throw_type_error(env, NULL, "bbq_napi: option name must be a string"); return NULL; }
  if (!get_i64(env, a[2], &value)) return NULL;
  int rc = bbq_vectors_set_option(v, name, value);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* searchRerankBatch(index, vectors, nq, queries Float32Array, qquant Uint8Array, qcorr Float64Array, queryBits, sim, k, factor, selector, trueSim)
 *   -> {indices Int32Array[nq*k], quantized Float32Array[nq*k], trueScores Float64Array[nq*k], counts Float64Array[nq], stride} */
static napi_value SearchRerankBatch(napi_env env, napi_callback_info info) {
  napi_value a[12];
  if (!get_args(env, info, 12, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[1]);
  if (!v) return NULL;
  void *q, *qq, *qc; size_t fl, ql, cl;
  int64_t nq, qb, sim, k, factor, selector, tsim;
  if (!get_i64(env, a[2], &nq) || !get_typed(env, a[3], napi_float32_array, &q, &fl) || !get_typed(env, a[4], napi_uint8_array, &qq, &ql) ||
      !get_typed(env, a[5], napi_float64_array, &qc, &cl) || !get_i64(env, a[6], &qb) || !get_i64(env, a[7], &sim) || !get_i64(env, a[8], &k) ||
      !get_i64(env, a[9], &factor) || !get_i64(env, a[10], &selector) || !get_i64(env, a[11], &tsim)) return NULL;
  const size_t dim = (size_t)bbq_index_dimension(ix);
  if (nq < 0 || ql != (size_t)nq * dim || fl != (size_t)nq * dim || cl != (size_t)nq * 4) {
    napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL;
  }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  void *oi, *oq, *ot, *on;
  napi_value ti = new_typed(env, napi_int32_array, (size_t)(nq * k), 4, &oi);
  napi_value tq = new_typed(env, napi_float32_array, (size_t)(nq * k), 4, &oq);
  napi_value tt = new_typed(env, napi_float64_array, (size_t)(nq * k), 8, &ot);
  napi_value tn = new_typed(env, napi_float64_array, (size_t)nq, 8, &on);
  if (!ti || !tq || !tt || !tn) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t *cnt = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
  int rc = bbq_search_rerank_batch(ix, v, (int32_t)nq, (const float *)q, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, k,
                                   (int32_t)factor, (int32_t)selector, (int32_t)tsim, (int32_t *)oi, (float *)oq, (double *)ot, cnt);
  if (rc != BBQ_OK) { free(cnt); return throw_bbq(env, rc); }
  for (int64_t i = 0; i < nq; ++i) ((double *)on)[i] = (double)cnt[i];
  free(cnt);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "indices", ti); set_prop(env, o, "quantized", tq); set_prop(env, o, "trueScores", tt); set_prop(env, o, "counts", tn);
  napi_value kv; napi_create_double(env, (double)k, &kv); set_prop(env, o, "stride", kv);
  return o;
}

/* the group set of the exact MaxSim rerank calls */
static const bbq_groups *unbox_groups(napi_env env, napi_value v, const char *fn) {
  void *gp = NULL;
  if (napi_get_value_external(env, v, &gp) != napi_ok || !gp || !*(bbq_groups **)gp) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: the group set is null", fn);
    napi_throw_error(env, "BBQ1", msg);
    return NULL;
  }
  return *(bbq_groups **)gp;
}

/* rerankMaxSimGroups(vectors, groups handle, tokens Float32Array[T * dim], trueSim, candidates Int32Array) -> Float64Array: the exact MaxSim
 * score of every candidate group, in list order, for ONE query of T >= 1 raw token vectors (bbq_rerank_maxsim_groups_batch with one query) */
static napi_value RerankMaxSimGroups(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!get_args(env, info, 5, a)) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[0]);
  if (!v) return NULL;
  const bbq_groups *grp = unbox_groups(env, a[1], "bbq_rerank_maxsim_groups_batch");
  if (!grp) return NULL;
  void *q, *cg; size_t ql, nc;
  int64_t sim;
  if (!get_typed(env, a[2], napi_float32_array, &q, &ql) || !get_i64(env, a[3], &sim) || !get_typed(env, a[4], napi_int32_array, &cg, &nc)) return NULL;
  const size_t dim = (size_t)bbq_vectors_dimension(v);
  if (dim == 0 || ql == 0 || ql % dim != 0) { napi_throw_error(env, "BBQ6", "向量维度不匹配"); return NULL; }
  const int64_t voff[2] = {0, (int64_t)(ql / dim)}, coff[2] = {0, (int64_t)nc};
  void *out;
  napi_value t = new_typed(env, napi_float64_array, nc, 8, &out);
  if (!t) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_rerank_maxsim_groups_batch(v, grp, 1, voff, (const float *)q, (int32_t)sim, coff, (const int32_t *)cg, (double *)out);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  return t;
}

/* searchMaxSimRerank(index, vectors, groups handle, tokens Float32Array[T * dim], qquant Uint8Array[T * dim], qcorr Float64Array[T * 4], queryBits,
 * sim, k, factor, selector, trueSim) -> {groups Int32Array, quantized Float32Array, trueScores Float64Array}: the whole recipe for ONE query
 * (bbq_search_maxsim_rerank_batch with one query) */
static napi_value SearchMaxSimRerank(napi_env env, napi_callback_info info) {
  napi_value a[12];
  if (!get_args(env, info, 12, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  bbq_vectors *v = unbox_vectors(env, a[1]);
  if (!v) return NULL;
  const bbq_groups *grp = unbox_groups(env, a[2], "bbq_search_maxsim_rerank_batch");
  if (!grp) return NULL;
  void *q, *qq, *qc; size_t fl, ql, cl;
  int64_t qb, sim, k, factor, selector, tsim;
  if (!get_typed(env, a[3], napi_float32_array, &q, &fl) || !get_typed(env, a[4], napi_uint8_array, &qq, &ql) ||
      !get_typed(env, a[5], napi_float64_array, &qc, &cl) || !get_i64(env, a[6], &qb) || !get_i64(env, a[7], &sim) || !get_i64(env, a[8], &k) ||
      !get_i64(env, a[9], &factor) || !get_i64(env, a[10], &selector) || !get_i64(env, a[11], &tsim)) return NULL;
  const size_t dim = (size_t)bbq_index_dimension(ix);
  if (dim == 0 || ql == 0 || ql % dim != 0 || fl != ql || cl != ql / dim * 4) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  if (k < 0) { napi_throw_error(env, "BBQ7", "k值不能为负数"); return NULL; }
  const int64_t live = bbq_groups_live(grp);
  const int64_t keff = k < live ? k : live;   /* no answer is longer than the live groups */
  const int64_t voff[2] = {0, (int64_t)(ql / dim)};
  int32_t *og = (int32_t *)malloc(((size_t)keff + 1) * sizeof(int32_t));
  float *sq = (float *)malloc(((size_t)keff + 1) * sizeof(float));
  double *st = (double *)malloc(((size_t)keff + 1) * sizeof(double));
  if (!og || !sq || !st) { free(og); free(sq); free(st); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int64_t cnt = 0;
  int rc = bbq_search_maxsim_rerank_batch(ix, v, grp, 1, voff, (const float *)q, (const uint8_t *)qq, (const double *)qc, (int32_t)qb, (int32_t)sim, keff,
                                          (int32_t)factor, (int32_t)selector, (int32_t)tsim, og, sq, st, &cnt);
  if (rc != BBQ_OK) { free(og); free(sq); free(st); return throw_bbq(env, rc); }
  void *pg, *pq, *pt;
  napi_value tg = new_typed(env, napi_int32_array, (size_t)cnt, 4, &pg);
  napi_value tq = new_typed(env, napi_float32_array, (size_t)cnt, 4, &pq);
  napi_value tt = new_typed(env, napi_float64_array, (size_t)cnt, 8, &pt);
  if (!tg || !tq || !tt) { free(og); free(sq); free(st); napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  if (cnt > 0) { memcpy(pg, og, (size_t)cnt * 4); memcpy(pq, sq, (size_t)cnt * 4); memcpy(pt, st, (size_t)cnt * 8); }
  free(og); free(sq); free(st);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "groups", tg); set_prop(env, o, "quantized", tq); set_prop(env, o, "trueScores", tt);
  return o;
}

/* ---- on-disk format (bbq_index_save / bbq_index_load / bbq_index_export) */
static int get_path(napi_env env, napi_value v, char *buf, size_t cap) {
  size_t len = 0;
  if (napi_get_value_string_utf8(env, v, buf, cap, &len) != napi_ok || len == 0 || len >= cap - 1) {
    napi_throw_type_error(env, NULL, "bbq_napi: path string expected");
    return 0;
  }
  return 1;
}

/* indexSave(handle, prefix, centroid Float32Array, sim) */
static napi_value IndexSave(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!get_args(env, info, 4, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  char path[4096]; void *cen; size_t cl; int64_t sim;
  if (!get_path(env, a[1], path, sizeof path) || !get_typed(env, a[2], napi_float32_array, &cen, &cl) || !get_i64(env, a[3], &sim)) return NULL;
  if (cl != (size_t)bbq_index_dimension(ix)) { napi_throw_error(env, "BBQ6", "向量和质心维度不匹配"); return NULL; }
  int rc = bbq_index_save(ix, path, (const float *)cen, (int32_t)sim);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* indexLoad(prefix, device[, devices Int32Array]) -> {handle, centroid Float32Array, n, dim, sim, centroidDP, rowBase, shards, indexBits}
 * devices given and the files hold a multi-device index (a manifest): its shards go over those devices (bbq_index_load_multi) */
static napi_value IndexLoad(napi_env env, napi_callback_info info) {
  napi_value a[3];
  size_t argc = 3;
  if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 2) { napi_throw_type_error(env, NULL, "bbq_napi: wrong number of arguments"); return NULL; }
  char path[4096]; int64_t dev;
  if (!get_path(env, a[0], path, sizeof path) || !get_i64(env, a[1], &dev)) return NULL;
  void *devs = NULL; size_t ndevs = 0;
  if (argc >= 3) {
    napi_valuetype vt;
    if (napi_typeof(env, a[2], &vt) == napi_ok && vt != napi_undefined && vt != napi_null && !get_typed(env, a[2], napi_int32_array, &devs, &ndevs)) return NULL;
  }
  int64_t n = 0, rb = 0; int32_t dim = 0, sim = 0; double cdp = 0;
  int rc = bbq_index_file_info(path, &n, &dim, &sim, &cdp, &rb);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  void *cen;
  napi_value tcen = new_typed(env, napi_float32_array, (size_t)dim, 4, &cen);
  if (!tcen) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  bbq_index **box = (bbq_index **)calloc(1, sizeof *box);
  const int32_t file_shards = bbq_index_file_shards(path);
  if (devs && ndevs > 0 && file_shards > 1) rc = bbq_index_load_multi(path, (int32_t)ndevs, (const int32_t *)devs, box, (float *)cen);
  else rc = bbq_index_load(path, (int32_t)dev, box, (float *)cen);
  if (rc != BBQ_OK) { free(box); return throw_bbq(env, rc); }
  napi_value ext, o, v;
  if (napi_create_external(env, box, finalize_index, NULL, &ext) != napi_ok) { bbq_index_destroy(*box); free(box); napi_throw_error(env, NULL, "bbq_napi: external"); return NULL; }
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "handle", ext); set_prop(env, o, "centroid", tcen);
  napi_create_double(env, (double)n, &v); set_prop(env, o, "n", v);
  napi_create_double(env, (double)dim, &v); set_prop(env, o, "dim", v);
  napi_create_double(env, (double)sim, &v); set_prop(env, o, "sim", v);
  napi_create_double(env, cdp, &v); set_prop(env, o, "centroidDP", v);
  napi_create_double(env, (double)rb, &v); set_prop(env, o, "rowBase", v);
  napi_create_double(env, (double)file_shards, &v); set_prop(env, o, "shards", v);
  napi_create_double(env, (double)bbq_index_bits(*box), &v); set_prop(env, o, "indexBits", v);
  return o;
}

/* indexExport(handle) -> {codes Uint8Array[n*ceil(dim/8)], corr Float64Array[n*4]} */
static napi_value IndexExport(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  bbq_index *ix = unbox(env, a[0]);
  if (!ix) return NULL;
  const size_t dimx = (size_t)bbq_index_dimension(ix);
  const size_t n = (size_t)bbq_index_size(ix), pb = bbq_index_bits(ix) == 1 ? (dimx + 7) / 8 : dimx;
  void *codes, *corr;
  napi_value tcodes = new_typed(env, napi_uint8_array, n * pb, 1, &codes);
  napi_value tcorr = new_typed(env, napi_float64_array, n * 4, 8, &corr);
  if (!tcodes || !tcorr) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_index_export(ix, (uint8_t *)codes, (double *)corr);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "codes", tcodes); set_prop(env, o, "corr", tcorr);
  return o;
}

/* quantizeQueries(flat Float32Array[n*dim], n, centroid Float32Array[dim], sim, queryBits, lambda, iters, threads)
 *   -> {quantized Uint8Array[n*dim], corrections Float64Array[n*4]}   (bbq_quantize_queries: host threads) */
static napi_value QuantizeQueries(napi_env env, napi_callback_info info) {
  napi_value a[8];
  if (!get_args(env, info, 8, a)) return NULL;
  void *q, *cen; size_t ql, cl;
  int64_t n, sim, qb, iters, threads; double lambda;
  if (!get_typed(env, a[0], napi_float32_array, &q, &ql) || !get_i64(env, a[1], &n) || !get_typed(env, a[2], napi_float32_array, &cen, &cl) ||
      !get_i64(env, a[3], &sim) || !get_i64(env, a[4], &qb) || !get_f64(env, a[5], &lambda) || !get_i64(env, a[6], &iters) ||
      !get_i64(env, a[7], &threads)) return NULL;
  if (n < 0 || cl == 0 || ql != (size_t)n * cl) { napi_throw_error(env, "BBQ6", "查询向量维度与目标向量维度不匹配"); return NULL; }
  void *oq, *oc;
  napi_value tq = new_typed(env, napi_uint8_array, ql, 1, &oq);
  napi_value tc = new_typed(env, napi_float64_array, (size_t)n * 4, 8, &oc);
  if (!tq || !tc) { napi_throw_error(env, NULL, "bbq_napi: allocation failed"); return NULL; }
  int rc = bbq_quantize_queries((const float *)q, (int32_t)n, (int32_t)cl, (const float *)cen, (int32_t)sim, (int32_t)qb, lambda, (int32_t)iters,
                                (int32_t)threads, (uint8_t *)oq, (double *)oc, NULL);
  if (rc != BBQ_OK) return throw_bbq(env, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_prop(env, o, "quantized", tq); set_prop(env, o, "corrections", tc);
  return o;
}

static napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor d[] = {
      {"deviceCount", NULL, DeviceCount, NULL, NULL, NULL, napi_default, NULL},
      {"quantizeVectors", NULL, QuantizeVectors, NULL, NULL, NULL, napi_default, NULL},
      {"quantizeQuery", NULL, QuantizeQuery, NULL, NULL, NULL, napi_default, NULL},
      {"quantizeQueries", NULL, QuantizeQueries, NULL, NULL, NULL, napi_default, NULL},
      {"centroidDP", NULL, CentroidDP, NULL, NULL, NULL, napi_default, NULL},
      {"indexCreate", NULL, IndexCreate, NULL, NULL, NULL, napi_default, NULL},
      {"indexCreateMulti", NULL, IndexCreateMulti, NULL, NULL, NULL, napi_default, NULL},
      {"indexBuild", NULL, IndexBuild, NULL, NULL, NULL, napi_default, NULL},
      {"indexDestroy", NULL, IndexDestroy, NULL, NULL, NULL, napi_default, NULL},
      {"quantizeRows", NULL, QuantizeRows, NULL, NULL, NULL, napi_default, NULL},
      {"indexAppend", NULL, IndexAppend, NULL, NULL, NULL, napi_default, NULL},
      {"indexAppendRows", NULL, IndexAppendRows, NULL, NULL, NULL, napi_default, NULL},
      {"indexUpdate", NULL, IndexUpdate, NULL, NULL, NULL, napi_default, NULL},
      {"indexUpdateRows", NULL, IndexUpdateRows, NULL, NULL, NULL, napi_default, NULL},
      {"updateWinners", NULL, UpdateWinners, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsUpdate", NULL, VectorsUpdate, NULL, NULL, NULL, napi_default, NULL},
      {"indexReserve", NULL, IndexReserve, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsAppend", NULL, VectorsAppend, NULL, NULL, NULL, napi_default, NULL},
      {"indexCompact", NULL, IndexCompact, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsCompact", NULL, VectorsCompact, NULL, NULL, NULL, napi_default, NULL},
      {"searchBatch", NULL, SearchBatch, NULL, NULL, NULL, napi_default, NULL},
      {"filterCreate", NULL, FilterCreate, NULL, NULL, NULL, napi_default, NULL},
      {"filterDestroy", NULL, FilterDestroy, NULL, NULL, NULL, napi_default, NULL},
      {"searchFilteredBatch", NULL, SearchFilteredBatch, NULL, NULL, NULL, napi_default, NULL},
      {"searchRawBatch", NULL, SearchRawBatch, NULL, NULL, NULL, napi_default, NULL},
      {"searchRawInto", NULL, SearchRawInto, NULL, NULL, NULL, napi_default, NULL},
      {"scoreRows", NULL, ScoreRows, NULL, NULL, NULL, napi_default, NULL},
      {"scoreOrds", NULL, ScoreOrds, NULL, NULL, NULL, napi_default, NULL},
      {"searchOrds", NULL, SearchOrds, NULL, NULL, NULL, napi_default, NULL},
      {"searchRange", NULL, SearchRange, NULL, NULL, NULL, napi_default, NULL},
      {"searchSpans", NULL, SearchSpans, NULL, NULL, NULL, napi_default, NULL},
      {"searchSpansFiltered", NULL, SearchSpansFiltered, NULL, NULL, NULL, napi_default, NULL},
      {"groupsCreate", NULL, GroupsCreate, NULL, NULL, NULL, napi_default, NULL},
      {"groupsDestroy", NULL, GroupsDestroy, NULL, NULL, NULL, napi_default, NULL},
      {"searchGrouped", NULL, SearchGrouped, NULL, NULL, NULL, napi_default, NULL},
      {"searchMaxSim", NULL, SearchMaxSim, NULL, NULL, NULL, napi_default, NULL},
      {"scoreMaxSimGroups", NULL, ScoreMaxSimGroups, NULL, NULL, NULL, napi_default, NULL},
      {"searchMaxSimGroups", NULL, SearchMaxSimGroups, NULL, NULL, NULL, napi_default, NULL},
      {"setOption", NULL, SetOption, NULL, NULL, NULL, napi_default, NULL},
      {"stats", NULL, Stats, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsCreate", NULL, VectorsCreate, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsDestroy", NULL, VectorsDestroy, NULL, NULL, NULL, napi_default, NULL},
      {"rerankScores", NULL, RerankScores, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsSearchBatch", NULL, VectorsSearchBatch, NULL, NULL, NULL, napi_default, NULL},
      {"vectorsSetOption", NULL, VectorsSetOption, NULL, NULL, NULL, napi_default, NULL},
      {"searchRerankBatch", NULL, SearchRerankBatch, NULL, NULL, NULL, napi_default, NULL},
      {"rerankMaxSimGroups", NULL, RerankMaxSimGroups, NULL, NULL, NULL, napi_default, NULL},
      {"searchMaxSimRerank", NULL, SearchMaxSimRerank, NULL, NULL, NULL, napi_default, NULL},
      {"indexSave", NULL, IndexSave, NULL, NULL, NULL, napi_default, NULL},
      {"indexLoad", NULL, IndexLoad, NULL, NULL, NULL, napi_default, NULL},
      {"indexExport", NULL, IndexExport, NULL, NULL, NULL, napi_default, NULL},
  };
  if (napi_define_properties(env, exports, sizeof d / sizeof d[0], d) != napi_ok) return NULL;
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
