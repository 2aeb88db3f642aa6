"""Python mirror of the reference's public surface for the search path (same names, argument meaning and error
behaviour as src/index.ts:47-111 and src/binaryQuantizationFormat.ts:132-412), implemented entirely on libbbq."""
import weakref

import numpy as np

from . import capi


class VectorSimilarityFunction:  # src/types.ts:9-13 (string enum)
    EUCLIDEAN = "EUCLIDEAN"
    COSINE = "COSINE"
    MAXIMUM_INNER_PRODUCT = "MAXIMUM_INNER_PRODUCT"


DEFAULT_CONFIG = {"queryBits": 4, "indexBits": 1,
                  "quantizer": {"similarityFunction": VectorSimilarityFunction.COSINE, "lambda": 0.1, "iters": 5}}


class BinarizedByteVectorValues:
    """src/types.ts:32-49 / BinarizedByteVectorValuesImpl (src/binaryQuantizationFormat.ts:24-126): flat arrays with
    per-row views; the device copy is created lazily on first search and cached on the object."""

    def __init__(self, codes, corr, centroid, index_bits):
        self._codes, self._corr, self._centroid, self._index_bits = codes, corr, centroid, index_bits
        self._device_index = None

    def dimension(self):
        return int(self._centroid.shape[0])

    def size(self):
        return int(self._codes.shape[0])

    def vectorValue(self, ord_):
        if not 0 <= ord_ < self.size():
            raise Exception("向量索引 %d 不存在" % ord_)
        return self._codes[ord_]

    def getCorrectiveTerms(self, ord_):
        if not 0 <= ord_ < self.size():
            raise Exception("修正项索引 %d 不存在" % ord_)
        c = self._corr[ord_]
        return {"lowerInterval": float(c[0]), "upperInterval": float(c[1]), "additionalCorrection": float(c[2]),
                "quantizedComponentSum": float(c[3])}

    def getCentroid(self):
        return self._centroid

    def getCentroidDP(self, queryVector=None):
        if queryVector is not None:
            q = np.asarray(queryVector, np.float32).astype(np.float64)
            return float(np.sum(q * self._centroid.astype(np.float64)))  # unused by the search path
        return capi.centroid_dp(self._centroid)

    def _device(self, device=0):
        if self._device_index is None:
            self._device_index = capi.Index(self._codes, self._corr, self.dimension(), self.getCentroidDP(), device=device,
                                            index_bits=self._index_bits)
        return self._device_index


class BinaryQuantizationFormat:
    def __init__(self, config):
        qb = config.get("queryBits")
        ib = config.get("indexBits")
        if qb is not None and (qb < 1 or qb > 8):
            raise Exception("queryBits必须在1-8之间")
        if ib is not None and (ib < 1 or ib > 8):
            raise Exception("indexBits必须在1-8之间")
        self._config = {"queryBits": 4, "indexBits": 1}
        self._config.update(config)
        qz = config["quantizer"]
        self._sim = qz.get("similarityFunction", VectorSimilarityFunction.EUCLIDEAN)
        self._lambda = qz.get("lambda", 0.1)
        self._iters = qz.get("iters", 5)

    def getConfig(self):
        return self._config

    def quantizeVectors(self, vectors):
        if len(vectors) == 0:
            raise Exception("向量集合不能为空")
        dim = len(vectors[0])
        for i, v in enumerate(vectors):
            if len(v) != dim:
                raise Exception("向量 %d 维度 %d 与第一个向量维度 %d 不匹配" % (i, len(v), dim))
        try:
            if capi.device_count() > 0:
                # quantizeVectors as HIP kernels; the device index is ready when this returns
                ix, codes, corr, cen = capi.Index.build(np.asarray(vectors, np.float32), capi.SIMS[self._sim], self._lambda, self._iters,
                                                        index_bits=self._config["indexBits"])
                values = BinarizedByteVectorValues(codes, corr, cen, self._config["indexBits"])
                values._device_index = ix
            else:
                codes, corr, cen = capi.quantize_vectors(np.asarray(vectors, np.float32), capi.SIMS[self._sim],
                                                         self._config["indexBits"], self._lambda, self._iters)
                values = BinarizedByteVectorValues(codes, corr, cen, self._config["indexBits"])
        except capi.BBQError as e:
            raise Exception(str(e))
        return {"quantizedVectors": values, "queryQuantizer": self}

    def appendVectors(self, targetVectors, vectors):
        """extension: `vectors` quantized against targetVectors' centroid - quantizeVectors' per-row part (normalizeVector for COSINE,
        validation, scalarQuantize, packAsBinary) - become its next ords: size(), vectorValue, getCorrectiveTerms and every search
        cover them.  On the device when there is one (the resident index grows in place), on the host otherwise.  Returns targetVectors."""
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if len(vectors) == 0:
            return targetVectors
        dim = targetVectors.dimension()
        for i, v in enumerate(vectors):
            if len(v) != dim:
                raise Exception("向量 %d 维度 %d 与第一个向量维度 %d 不匹配" % (i, len(v), dim))
        if targetVectors._index_bits != self._config["indexBits"]:
            raise Exception("indexBits %d 与目标向量集合的 %d 不匹配" % (self._config["indexBits"], targetVectors._index_bits))
        v = np.asarray(vectors, np.float32)
        sim = capi.SIMS[self._sim]
        try:
            if capi.device_count() > 0:
                codes, corr = targetVectors._device().append(v, targetVectors.getCentroid(), sim, self._lambda, self._iters)
            else:
                codes, corr = capi.quantize_rows(v, targetVectors.getCentroid(), sim, targetVectors._index_bits, self._lambda, self._iters)
        except capi.BBQError as e:
            raise Exception(str(e))
        # the host copies behind size() / vectorValue / getCorrectiveTerms follow (new arrays: rows handed out earlier stay valid)
        targetVectors._codes = np.concatenate([targetVectors._codes, codes])
        targetVectors._corr = np.concatenate([targetVectors._corr, corr])
        return targetVectors

    def updateVectors(self, targetVectors, ords, vectors):
        """extension: `vectors` quantized against targetVectors' centroid - as appendVectors quantizes them - REPLACE the rows `ords`
        in place; among equal ords the last one wins.  The size and every ord stay, so row filters made earlier stay valid.  On the
        device when there is one (bbq_index_update), on the host otherwise.  Returns targetVectors."""
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        o = np.asarray(ords, np.int64).ravel()
        if len(vectors) != o.shape[0]:
            raise Exception("ords 数量 %d 与向量数量 %d 不匹配" % (o.shape[0], len(vectors)))
        if len(vectors) == 0:
            return targetVectors
        dim = targetVectors.dimension()
        for i, v in enumerate(vectors):
            if len(v) != dim:
                raise Exception("向量 %d 维度 %d 与第一个向量维度 %d 不匹配" % (i, len(v), dim))
        if targetVectors._index_bits != self._config["indexBits"]:
            raise Exception("indexBits %d 与目标向量集合的 %d 不匹配" % (self._config["indexBits"], targetVectors._index_bits))
        bad = o[(o < 0) | (o >= targetVectors.size())]
        if bad.size:
            raise Exception("向量索引 %d 不存在" % int(bad[0]))
        v = np.asarray(vectors, np.float32)
        sim = capi.SIMS[self._sim]
        try:
            if capi.device_count() > 0:
                codes, corr = targetVectors._device().update(o, v, targetVectors.getCentroid(), sim, self._lambda, self._iters)
            else:
                codes, corr = capi.quantize_rows(v, targetVectors.getCentroid(), sim, targetVectors._index_bits, self._lambda, self._iters)
            win = capi.update_winners(o, targetVectors.size())
        except capi.BBQError as e:
            raise Exception(str(e))
        # the host copies follow (new arrays: rows handed out earlier stay valid)
        targetVectors._codes, targetVectors._corr = targetVectors._codes.copy(), targetVectors._corr.copy()
        targetVectors._codes[o[win]] = codes[win]
        targetVectors._corr[o[win]] = corr[win]
        return targetVectors

    def compactVectors(self, targetVectors, accept):
        """extension: targetVectors becomes the set over the rows `accept` keeps - a bool mask of length size(), an array of ords, or
        a predicate ord -> bool - in order: the new ord of old row r is the number of kept rows below r.  The resident index is
        compacted on the device (bbq_index_compact; the rows do not leave it) and the host copies follow; without a device the host
        copies alone.  Row filters made earlier no longer fit.  Returns targetVectors."""
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        n = targetVectors.size()
        if callable(accept):
            accept = np.fromiter((bool(accept(i)) for i in range(n)), np.bool_, n)
        a = np.asarray(accept)
        if a.dtype != np.bool_:
            ords = np.asarray(a, np.int64).ravel()
            bad = ords[(ords < 0) | (ords >= n)]
            if bad.size:
                raise Exception("向量索引 %d 不存在" % int(bad[0]))
            a = np.zeros(n, np.bool_)
            a[ords] = True
        if a.shape != (n,):
            raise Exception("a filter mask has one entry per row of the index")
        try:
            if targetVectors._device_index is not None:   # never a stale device copy: it is compacted with the host rows
                with capi.Filter(targetVectors._device_index, a) as flt:
                    targetVectors._device_index.compact(flt)
            kept = capi.kept_rows(a)
        except capi.BBQError as e:
            raise Exception(str(e))
        targetVectors._codes = targetVectors._codes[kept]
        targetVectors._corr = targetVectors._corr[kept]
        return targetVectors

    def removeVectors(self, targetVectors, ords):
        """extension: drop the rows `ords` (any order, duplicates allowed): compactVectors over the complement"""
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        n = targetVectors.size()
        o = np.asarray(ords, np.int64).ravel()
        bad = o[(o < 0) | (o >= n)]
        if bad.size:
            raise Exception("向量索引 %d 不存在" % int(bad[0]))
        keep = np.ones(n, np.bool_)
        keep[o] = False
        return self.compactVectors(targetVectors, keep)

    def quantizeQueryVector(self, queryVector, centroid):
        qq, qc = capi.quantize_query(queryVector, centroid, capi.SIMS[self._sim], self._config["queryBits"], self._lambda,
                                     self._iters, search_path=False)
        return {"quantizedQuery": qq, "queryCorrections": {"lowerInterval": qc[0], "upperInterval": qc[1],
                                                          "additionalCorrection": qc[2], "quantizedComponentSum": qc[3]}}

    def searchNearestNeighbors(self, queryVector, targetVectors, k):
        return self._search(queryVector, targetVectors, k, None)

    def searchNearestNeighborsFiltered(self, queryVector, targetVectors, rowFilter, k):
        """extension: searchNearestNeighbors over the rows `rowFilter` (createRowFilter) accepts - what the reference's loop
        returns when it visits only those ords, ascending"""
        if rowFilter is None:
            raise Exception("行过滤器不能为空")
        return self._search(queryVector, targetVectors, k, rowFilter)

    def searchNearestNeighborsInOrds(self, queryVector, targetVectors, ords, k):
        """extension: searchNearestNeighbors over exactly the rows `ords` names - what the reference's loop returns when it visits
        those ords in the order given (any order, duplicates allowed), with a heap of min(k, len(ords)).  The list may differ from
        query to query, which a row filter cannot; the device scores only the rows named."""
        if ords is None:
            raise Exception("目标向量序号不能为空")
        return self._search(queryVector, targetVectors, k, None, ords)

    def searchNearestNeighborsInSpans(self, queryVector, targetVectors, spans, k):
        """extension: searchNearestNeighbors over the rows of `spans` - a list of (begin, end) pairs, end exclusive, ascending and
        disjoint; empty spans and an empty list are allowed - what the reference's loop returns when it visits exactly those rows,
        ascending, with a heap of min(k, rows visited).  The spans may differ from query to query, which a row filter cannot; the
        device streams them as whole tiles and selects the k best itself."""
        if spans is None:
            raise Exception("行区间不能为空")
        return self._search(queryVector, targetVectors, k, None, None, np.asarray(spans, np.int64).reshape(-1, 2))

    def searchNearestNeighborsInSpansFiltered(self, queryVector, targetVectors, spans, rowFilter, k):
        """extension: searchNearestNeighborsInSpans over the rows `rowFilter` (createRowFilter) accepts - what the reference's loop
        returns when it visits exactly the accepted rows of the spans, ascending, with a heap of min(k, accepted rows visited): deleted
        rows, one tenant's rows or a metadata predicate in a store that keeps its rows cluster by cluster."""
        if spans is None:
            raise Exception("行区间不能为空")
        if rowFilter is None:
            raise Exception("行过滤器不能为空")
        return self._search(queryVector, targetVectors, k, rowFilter, None, np.asarray(spans, np.int64).reshape(-1, 2))

    def searchNearestNeighborsGrouped(self, queryVector, targetVectors, rowGroups, k):
        """extension: the k best groups of `rowGroups` (createRowGroups) - documents held as runs of chunk rows - each through its best
        accepted row: what the reference's loop returns when it visits exactly each live group's best row, ascending, with a heap of
        min(k, live groups).  Returns [{index, score, group}]."""
        if queryVector is None:
            raise Exception("查询向量不能为空")
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if rowGroups is None:
            raise Exception("行分组不能为空")
        if k < 0:
            raise Exception("k值不能为负数")
        if len(queryVector) != targetVectors.dimension():
            raise Exception("查询向量维度与目标向量维度不匹配")
        if k == 0:
            return []
        sim = capi.SIMS[self._sim]
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and self._config["queryBits"] not in (1, 4):
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % self._config["queryBits"])  # as _search refuses it
        try:
            qq, qc = capi.quantize_query(queryVector, targetVectors.getCentroid(), sim, self._config["queryBits"], self._lambda,
                                         self._iters, search_path=True)
            idx, sc, grp = targetVectors._device().search_grouped_batch(qq[None, :], qc[None, :], self._config["queryBits"], sim, k, rowGroups)[0][0]
        except capi.BBQError as e:
            raise Exception(str(e))
        return [{"index": int(i), "score": float(s), "group": int(g)} for i, s, g in zip(idx, sc, grp)]

    def searchNearestNeighborsMaxSim(self, queryVectors, targetVectors, rowGroups, k):
        """extension: the k best groups of `rowGroups` (createRowGroups) for a query that is a bag of token vectors - late interaction,
        MaxSim: a group scores the sum over the query's vectors, in their order, of its best accepted row's score for each.  What the
        reference's loop returns when it visits the live groups, ascending, with a heap of min(k, live groups).  Every vector is
        quantized the way searchNearestNeighborsGrouped quantizes its one.  Returns [{group, score}]."""
        if queryVectors is None or len(queryVectors) == 0:
            raise Exception("查询向量不能为空")
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if rowGroups is None:
            raise Exception("行分组不能为空")
        if k < 0:
            raise Exception("k值不能为负数")
        for v in queryVectors:
            if v is None:
                raise Exception("查询向量不能为空")
            if len(v) != targetVectors.dimension():
                raise Exception("查询向量维度与目标向量维度不匹配")
        if k == 0:
            return []
        sim = capi.SIMS[self._sim]
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and self._config["queryBits"] not in (1, 4):
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % self._config["queryBits"])  # as _search refuses it
        try:
            pairs = [capi.quantize_query(v, targetVectors.getCentroid(), sim, self._config["queryBits"], self._lambda, self._iters, search_path=True)
                     for v in queryVectors]
            tokens = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
            grp, sc = targetVectors._device().search_maxsim_batch([tokens], self._config["queryBits"], sim, k, rowGroups)[0][0]
        except capi.BBQError as e:
            raise Exception(str(e))
        return [{"group": int(g), "score": float(s)} for g, s in zip(grp, sc)]

    def searchNearestNeighborsMaxSimInGroups(self, queryVectors, targetVectors, rowGroups, groupNumbers, k):
        """extension: searchNearestNeighborsMaxSim over the candidate groups `groupNumbers` alone - the second stage of late interaction,
        behind a first stage that nominated them.  What the reference's loop returns when it visits exactly those groups of `rowGroups`,
        in the order given and a duplicate once per occurrence, with a heap of min(k, candidates).  Every candidate must be a live group.
        Returns [{group, score}]."""
        if queryVectors is None or len(queryVectors) == 0:
            raise Exception("查询向量不能为空")
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if rowGroups is None:
            raise Exception("行分组不能为空")
        if groupNumbers is None:
            raise Exception("候选分组不能为空")
        if k < 0:
            raise Exception("k值不能为负数")
        for v in queryVectors:
            if v is None:
                raise Exception("查询向量不能为空")
            if len(v) != targetVectors.dimension():
                raise Exception("查询向量维度与目标向量维度不匹配")
        sim = capi.SIMS[self._sim]
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and self._config["queryBits"] not in (1, 4):
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % self._config["queryBits"])  # as _search refuses it
        try:
            pairs = [capi.quantize_query(v, targetVectors.getCentroid(), sim, self._config["queryBits"], self._lambda, self._iters, search_path=True)
                     for v in queryVectors]
            tokens = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
            cand = np.asarray(groupNumbers, np.int64).reshape(-1)
            grp, sc = targetVectors._device().search_maxsim_groups_batch([tokens], self._config["queryBits"], sim, k, rowGroups, [cand])[0]
        except capi.BBQError as e:
            raise Exception(str(e))
        return [{"group": int(g), "score": float(s)} for g, s in zip(grp, sc)]

    def searchNearestNeighborsMaxSimReranked(self, queryVectors, targetVectors, vectors, rowGroups, k, oversampleFactor, selector="heap"):
        """extension: the late-interaction recall recipe - searchNearestNeighborsMaxSim with k * oversampleFactor, the exact MaxSim
        scores of the returned groups on `vectors` (createDeviceVectors over the original rows; COSINE, as the reference's selectors),
        then the 'heap' or the 'sort' selector of getOversampledTopKWith{Heap,Sort} over the true scores.  Returns [{group,
        quantizedScore, trueScore}]."""
        if queryVectors is None or len(queryVectors) == 0:
            raise Exception("查询向量不能为空")
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if not isinstance(vectors, capi.Vectors):
            raise Exception("searchNearestNeighborsMaxSimReranked needs createDeviceVectors(vectors)")
        if rowGroups is None:
            raise Exception("行分组不能为空")
        if k < 0:
            raise Exception("k值不能为负数")
        for v in queryVectors:
            if v is None:
                raise Exception("查询向量不能为空")
            if len(v) != targetVectors.dimension():
                raise Exception("查询向量维度与目标向量维度不匹配")
        if k == 0:
            return []
        sim = capi.SIMS[self._sim]
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and self._config["queryBits"] not in (1, 4):
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % self._config["queryBits"])  # as _search refuses it
        try:
            pairs = [capi.quantize_query(v, targetVectors.getCentroid(), sim, self._config["queryBits"], self._lambda, self._iters, search_path=True)
                     for v in queryVectors]
            tokens = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
            raw = np.stack([np.asarray(v, np.float32) for v in queryVectors])
            grp, qs, ts = capi.search_maxsim_rerank_batch(targetVectors._device(), vectors, rowGroups, [raw], [tokens], self._config["queryBits"], sim, k,
                                                          oversampleFactor, 1 if selector == "sort" else 0, 1)[0]
        except capi.BBQError as e:
            raise Exception(str(e))
        return [{"group": int(g), "quantizedScore": float(q), "trueScore": float(t)} for g, q, t in zip(grp, qs, ts)]

    def searchRange(self, queryVector, targetVectors, threshold, rowFilter=None, order="ord"):
        """extension: every row (of `rowFilter`, createRowFilter, if given) whose stored f32 score is >= threshold - what the
        reference's loop would collect if it kept every visited ord at or above the threshold and skipped the heap - as
        [{index, score}] in ascending ord; order="score": descending score, ties in ascending ord.  A NaN score is in no answer;
        a NaN threshold raises."""
        if queryVector is None:
            raise Exception("查询向量不能为空")
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if order not in ("ord", "score"):
            raise Exception('order must be "ord" or "score"')
        if threshold is None or threshold != threshold:
            raise Exception("阈值不能为NaN")
        if len(queryVector) != targetVectors.dimension():
            raise Exception("查询向量维度与目标向量维度不匹配")
        sim = capi.SIMS[self._sim]
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and self._config["queryBits"] not in (1, 4):
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % self._config["queryBits"])  # as _search refuses it
        try:
            qq, qc = capi.quantize_query(queryVector, targetVectors.getCentroid(), sim, self._config["queryBits"], self._lambda,
                                         self._iters, search_path=True)
            idx, sc, _ = targetVectors._device().search_range_batch(qq[None, :], qc[None, :], self._config["queryBits"], sim, [threshold], rowFilter)
        except capi.BBQError as e:
            raise Exception(str(e))
        if order == "score":
            by = np.argsort(-sc, kind="stable")  # no NaN among them
            idx, sc = idx[by], sc[by]
        return [{"index": int(i), "score": float(s)} for i, s in zip(idx, sc)]

    def computeBatchQuantizedScores(self, quantizedQuery, queryCorrections, targetVectors, targetOrds, queryBits):
        """BinaryQuantizedScorer.computeBatchQuantizedScores (src/binaryQuantizedScorer.ts:315-420) without its optional
        originalQueryVector: [{score, bitDotProduct}] for the rows targetOrds names, in that order, scored on the device
        (bbq_score_ords: those rows and no others)"""
        if len(targetOrds) == 0:
            return []
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and queryBits not in (1, 4):
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % queryBits)
        qc = np.array([queryCorrections[f] for f in ("lowerInterval", "upperInterval", "additionalCorrection", "quantizedComponentSum")], np.float64)
        try:
            d, s64, _ = targetVectors._device().score_ords(quantizedQuery, qc, queryBits, capi.SIMS[self._sim], targetOrds, want=(True, True, False))
        except capi.BBQError as e:
            raise Exception(str(e))
        return [{"score": float(s), "bitDotProduct": int(b)} for s, b in zip(s64, d)]

    def _search(self, queryVector, targetVectors, k, rowFilter, ords=None, spans=None):
        if queryVector is None:
            raise Exception("查询向量不能为空")
        if targetVectors is None:
            raise Exception("目标向量集合不能为空")
        if k < 0:
            raise Exception("k值不能为负数")
        if len(queryVector) != targetVectors.dimension():
            raise Exception("查询向量维度与目标向量维度不匹配")
        if k == 0:
            return []
        sim = capi.SIMS[self._sim]
        if targetVectors._index_bits != 1 and targetVectors.dimension() > 1 and self._config["queryBits"] not in (1, 4):
            # the reference's batch scorer throws on a multi-bit index and its per-row fallback only knows 1- and 4-bit queries
            # (src/binaryQuantizedScorer.ts:95-97, :403-419); libbbq itself would score it (4-bit form, parity unpinned)
            raise Exception("不支持的查询位数: %d，只支持1位和4位" % self._config["queryBits"])
        try:
            qq, qc = capi.quantize_query(queryVector, targetVectors.getCentroid(), sim, self._config["queryBits"], self._lambda,
                                         self._iters, search_path=True)
            if spans is not None and rowFilter is not None:
                idx, sc = targetVectors._device().search_spans_filtered_batch(qq[None, :], qc[None, :], self._config["queryBits"], sim, k, [spans], rowFilter)[0][0]
            elif spans is not None:
                idx, sc = targetVectors._device().search_spans_batch(qq[None, :], qc[None, :], self._config["queryBits"], sim, k, [spans])[0][0]
            elif ords is not None:
                idx, sc = targetVectors._device().search_ords_batch(qq[None, :], qc[None, :], self._config["queryBits"], sim, k, [ords])[0]
            elif rowFilter is None:
                idx, sc = targetVectors._device().search(qq, qc, self._config["queryBits"], sim, k)
            else:
                idx, sc = targetVectors._device().search_filtered(qq, qc, self._config["queryBits"], sim, k, rowFilter)
        except capi.BBQError as e:
            raise Exception(str(e))
        return [{"index": int(i), "score": float(s)} for i, s in zip(idx, sc)]


def createBinaryQuantizationFormat(config=DEFAULT_CONFIG):
    return BinaryQuantizationFormat(config)


def quickQuantize(vectors, similarityFunction=VectorSimilarityFunction.COSINE):
    return BinaryQuantizationFormat({"quantizer": {"similarityFunction": similarityFunction, "lambda": 0.1, "iters": 5}}).quantizeVectors(vectors)


def quickSearch(queryVector, targetVectors, k, similarityFunction=VectorSimilarityFunction.COSINE):
    f = BinaryQuantizationFormat({"quantizer": {"similarityFunction": similarityFunction, "lambda": 0.1, "iters": 5}})
    return f.searchNearestNeighbors(queryVector, f.quantizeVectors(targetVectors)["quantizedVectors"], k)


def createRowFilter(targetVectors, accept):
    """extension: an accept set of `targetVectors` for searchNearestNeighborsFiltered; `accept` is a bool mask of length size(), an
    array of ords, or a predicate ord -> bool.  Returns a capi.Filter (.count, .close(), context manager)."""
    if callable(accept):
        accept = np.fromiter((bool(accept(i)) for i in range(targetVectors.size())), np.bool_, targetVectors.size())
    try:
        return capi.Filter(targetVectors._device(), accept)
    except capi.BBQError as e:
        raise Exception(str(e))


def createRowGroups(targetVectors, offsets, rowFilter=None):
    """extension: the groups of `targetVectors` for searchNearestNeighborsGrouped: group g is the rows [offsets[g], offsets[g + 1]),
    offsets[0] == 0, ascending, offsets[-1] == size(); `rowFilter` (createRowFilter) says which rows exist.  Returns a capi.Groups
    (.count, .live, .close(), context manager)."""
    if offsets is None:
        raise Exception("行分组不能为空")
    try:
        return capi.Groups(targetVectors._device(), offsets, rowFilter)
    except capi.BBQError as e:
        raise Exception(str(e))


def createDeviceVectors(vectors, device=0):
    """upload the original fp32 vectors once; pass the handle wherever the reference's selectors take `vectors`"""
    return capi.Vectors(np.asarray(vectors, np.float32), device)


def _oversampled(query, quantizedVectors, vectors, k, oversampleFactor, fmt, selector):
    # src/topKSelector.ts:29-115: searchNearestNeighbors(k*factor) -> computeCosineSimilarity per candidate -> select.
    # Search, true scores and selection all happen behind bbq_search_rerank_batch.
    oversampled = k * oversampleFactor
    if oversampled < 0:
        raise Exception("k值不能为负数")
    if len(query) != quantizedVectors.dimension():
        raise Exception("查询向量维度与目标向量维度不匹配")
    if oversampled == 0:
        return []
    owned = not isinstance(vectors, capi.Vectors)
    dv = createDeviceVectors(vectors) if owned else vectors
    try:
        sim = capi.SIMS[fmt._sim]
        q = np.ascontiguousarray(query, np.float32)
        qq, qc = capi.quantize_query(q, quantizedVectors.getCentroid(), sim, fmt._config["queryBits"], fmt._lambda, fmt._iters,
                                     search_path=True)
        idx, qs, ts, cnt = capi.search_rerank_batch(quantizedVectors._device(), dv, q[None, :], qq[None, :], qc[None, :],
                                                    fmt._config["queryBits"], sim, k, oversampleFactor, selector, 1)
    except capi.BBQError as e:
        raise Exception(str(e))
    finally:
        if owned:
            dv.close()
    return [{"index": int(idx[0, j]), "quantizedScore": float(qs[0, j]), "trueScore": float(ts[0, j])} for j in range(int(cnt[0]))]


def getOversampledTopKWithHeap(query, quantizedVectors, vectors, k, oversampleFactor, format):
    return _oversampled(query, quantizedVectors, vectors, k, oversampleFactor, format, 0)


def getOversampledTopKWithSort(query, quantizedVectors, vectors, k, oversampleFactor, format):
    return _oversampled(query, quantizedVectors, vectors, k, oversampleFactor, format, 1)


def getTrueTopK(query, vectors, k, similarity=VectorSimilarityFunction.COSINE, filter=None):
    """getTrueTopK, tests/recall-common.ts:143-149: the indices of the k rows of greatest similarity to `query`, equal scores in row
    order - every row scored in f64 and the k best selected on the device (bbq_vectors_search_batch).  `vectors`: a capi.Vectors
    (createDeviceVectors) or the rows themselves, uploaded for the call; `filter` (createRowFilter over the same rows): only the rows it
    accepts.  Returns a list of ints."""
    if k < 0:
        raise Exception("k值不能为负数")
    owned = not isinstance(vectors, capi.Vectors)
    dv = createDeviceVectors(vectors) if owned else vectors
    try:
        if similarity not in capi.SIMS:
            raise Exception("不支持的相似性函数: %s" % similarity)
        idx, _, cnt = dv.search_batch(np.ascontiguousarray(query, np.float32)[None, :], k, capi.SIMS[similarity], filter)
    except capi.BBQError as e:
        raise Exception(str(e))
    finally:
        if owned:
            dv.close()
    return [int(i) for i in idx[0, :int(cnt[0])]]
