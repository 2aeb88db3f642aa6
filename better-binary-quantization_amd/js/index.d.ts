// TypeScript surface of the MI355X drop-in (mirrors the reference's src/index.ts exports used on the search path).
export declare enum VectorSimilarityFunction { EUCLIDEAN = 'EUCLIDEAN', COSINE = 'COSINE', MAXIMUM_INNER_PRODUCT = 'MAXIMUM_INNER_PRODUCT' }
export interface QuantizationResult { lowerInterval: number; upperInterval: number; additionalCorrection: number; quantizedComponentSum: number; }
export interface QuantizerConfig { similarityFunction: VectorSimilarityFunction; lambda?: number; iters?: number; }
export interface BinaryQuantizationConfig { queryBits?: number; indexBits?: number; quantizer: QuantizerConfig; }
export interface BinarizedByteVectorValues {
  dimension(): number;
  vectorValue(ord: number): Uint8Array;
  getUnpackedVector(ord: number): Uint8Array;
  getCorrectiveTerms(ord: number): QuantizationResult;
  getCentroidDP(queryVector?: Float32Array): number;
  getCentroid(): Float32Array;
  size(): number;
  clearUnpackedVectorCache?(): void;
  /** releases the device-resident copy (extension) */
  dispose(): void;
  /** libbbq tuning knob on the device index, e.g. ('sweep_share', 32), ('resident_mb', 0) (extension; include/bbq.h lists them) */
  setDeviceOption(name: string, value: number): void;
  /** extension: room for `rows` rows in total on the device (appendVectors up to there moves nothing); returns the capacity in rows */
  reserve(rows: number): number;
  /** libbbq counters of the last call on the device index (extension; bbq_stats in include/bbq.h) */
  deviceStats(): { lastScanMs: number; lastScanBytes: number; candidates: number; denseFallbacks: number; hostReplays: number;
                   residentBytes: number; shards: number; bytesPerRow: number };
}
export interface QuantizedScoreResult { score: number; bitDotProduct: number; corrections: { query: QuantizationResult; index: QuantizationResult }; }
export declare class OptimizedScalarQuantizer {
  constructor(config: QuantizerConfig);
  scalarQuantize(vector: Float32Array, destination: Uint8Array, bits: number, centroid: Float32Array): QuantizationResult;
  multiScalarQuantize(vector: Float32Array, destinations: Uint8Array[], bits: number[], centroid: Float32Array): QuantizationResult[];
  static packAsBinary(vector: Uint8Array, packed: Uint8Array): void;
  static discretize(value: number, bucket: number): number;
  /** one byte per bit: quantQueryByte.length === q.length * 4 */
  static transposeHalfByte(q: Uint8Array, quantQueryByte: Uint8Array): void;
  static transposeHalfByteOptimized(q: Uint8Array, quantQueryByte: Uint8Array, useCache?: boolean): void;
  /** packed planes: quantQueryByte.length === ceil(q.length / 8) * 4 */
  static transposeHalfByteFast(q: Uint8Array, quantQueryByte: Uint8Array): void;
  static clearTransposeCache(): void;
  static getTransposeCacheStats(): { size: number; hitRate: number };
}
export declare class BinaryQuantizedScorer {
  constructor(similarityFunction: VectorSimilarityFunction);
  /** the single-row path of the reference (src/binaryQuantizedScorer.ts:69-301): host arithmetic, queryBits 1 or 4 */
  computeQuantizedScore(quantizedQuery: Uint8Array, queryCorrections: QuantizationResult, targetVectors: BinarizedByteVectorValues, targetOrd: number, queryBits: number, originalQueryVector?: Float32Array): QuantizedScoreResult;
  computeBatchQuantizedScores(quantizedQuery: Uint8Array, queryCorrections: QuantizationResult, targetVectors: BinarizedByteVectorValues,
    targetOrds: number[] | Int32Array, queryBits: number, originalQueryVector?: Float32Array): QuantizedScoreResult[];
  /** src/binaryQuantizedScorer.ts:429-617 */
  computeOriginalScore(originalQuery: Float32Array, targetVector: Float32Array, similarityFunction: VectorSimilarityFunction): number;
  compareScores(originalScore: number, quantizedScore: number): { difference: number; relativeError: number; correlation: number };
  computeQuantizationAccuracy(originalScores: number[], quantizedScores: number[]): { meanError: number; maxError: number; minError: number; stdError: number; correlation: number };
  getSimilarityFunction(): VectorSimilarityFunction;
}
export declare class BinaryQuantizationFormat {
  constructor(config: BinaryQuantizationConfig);
  quantizeVectors(vectors: Float32Array[]): { quantizedVectors: BinarizedByteVectorValues; queryQuantizer: OptimizedScalarQuantizer };
  /** extension: `vectors`, quantized against targetVectors' centroid like quantizeVectors quantizes its rows, become its next ords; the
   *  device index grows in place.  Not supported on a multi-device index (BBQ_DEVICES).  A RowFilter made before the call no longer
   *  fits the index.  Returns targetVectors. */
  appendVectors(targetVectors: BinarizedByteVectorValues, vectors: Float32Array[]): BinarizedByteVectorValues;
  /** extension: `vectors`, quantized against targetVectors' centroid as appendVectors quantizes them, replace the rows `ords` in place
   *  (the last of equal ords wins); size, ords and RowFilters made earlier stay valid.  Returns targetVectors. */
  updateVectors(targetVectors: BinarizedByteVectorValues, ords: Int32Array | number[], vectors: Float32Array[]): BinarizedByteVectorValues;
  /** extension: targetVectors becomes the set over the rows `filter` accepts, in order (new ord of old row r = accepted rows below r); a
   *  device copy is compacted on the device, the host copies follow.  `filter`: a RowFilter of targetVectors or anything createRowFilter
   *  takes.  Not supported on a multi-device index (BBQ_DEVICES).  The filter used and every RowFilter made earlier no longer fit the
   *  index.  Returns targetVectors. */
  compactVectors(targetVectors: BinarizedByteVectorValues, filter: RowFilter | Uint8Array | Int32Array | number[] | ((ord: number) => boolean)): BinarizedByteVectorValues;
  /** extension: drop the rows `ords` (any order, duplicates allowed): compactVectors over the complement.  Returns targetVectors. */
  removeVectors(targetVectors: BinarizedByteVectorValues, ords: ArrayLike<number>): BinarizedByteVectorValues;
  quantizeQueryVector(queryVector: Float32Array, centroid: Float32Array): { quantizedQuery: Uint8Array; queryCorrections: QuantizationResult };
  searchNearestNeighbors(queryVector: Float32Array, targetVectors: BinarizedByteVectorValues, k: number): Array<{ index: number; score: number }>;
  /** extension: many independent queries per call, pipelined on the device */
  searchNearestNeighborsBatch(queryVectors: Float32Array[], targetVectors: BinarizedByteVectorValues, k: number): Array<Array<{ index: number; score: number }>>;
  /** extension: searchNearestNeighbors over the ords `filter` accepts (what the reference's loop returns when it visits only those, ascending) */
  searchNearestNeighborsFiltered(query: Float32Array, targetVectors: BinarizedByteVectorValues, filter: RowFilter, k: number): Array<{ index: number; score: number }>;
  /** extension: searchNearestNeighbors over exactly the rows `ords` names, visited in the order given (any order, duplicates allowed); the list may differ from query to query */
  searchNearestNeighborsInOrds(query: Float32Array, targetVectors: BinarizedByteVectorValues, ords: Int32Array | number[], k: number): Array<{ index: number; score: number }>;
  /** extension: searchNearestNeighbors over the rows of `spans` - [begin, end) pairs, end exclusive, ascending and disjoint, empty spans and an empty list allowed; the spans may differ from query to query and the device selects the k best itself */
  searchNearestNeighborsInSpans(query: Float32Array, targetVectors: BinarizedByteVectorValues, spans: Array<[number, number]> | Float64Array, k: number): Array<{ index: number; score: number }>;
  /** extension: searchNearestNeighborsInSpans over the rows of the spans that `filter` accepts; the heap holds min(k, accepted rows visited) */
  searchNearestNeighborsInSpansFiltered(query: Float32Array, targetVectors: BinarizedByteVectorValues, spans: Array<[number, number]> | Float64Array, filter: RowFilter, k: number): Array<{ index: number; score: number }>;
  /** extension: the k best groups of `groups` (createRowGroups), each through its best accepted row - the reference's loop over each live group's best row, ascending, with a heap of min(k, live groups) */
  searchNearestNeighborsGrouped(query: Float32Array, targetVectors: BinarizedByteVectorValues, groups: RowGroups, k: number): Array<{ index: number; score: number; group: number }>;
  /** extension: the k best groups for a query of several token vectors (MaxSim, late interaction): a group scores the ordered sum of its best accepted row's score for every vector */
  searchNearestNeighborsMaxSim(queryVectors: Float32Array[], targetVectors: BinarizedByteVectorValues, groups: RowGroups, k: number): Array<{ group: number; score: number }>;
  /** extension: searchNearestNeighborsMaxSim over the candidate groups `groupNumbers` alone, visited in the order given, duplicates included; every candidate must be a live group */
  searchNearestNeighborsMaxSimInGroups(queryVectors: Float32Array[], targetVectors: BinarizedByteVectorValues, groups: RowGroups, groupNumbers: Int32Array | number[], k: number): Array<{ group: number; score: number }>;
  /** extension: the MaxSim score of every candidate group, in list order */
  computeMaxSimGroupScores(queryVectors: Float32Array[], targetVectors: BinarizedByteVectorValues, groups: RowGroups, groupNumbers: Int32Array | number[]): Float32Array;
  /** extension: every row (of options.rowFilter, if given) whose stored f32 score is >= threshold, in ascending ord or, with order 'score', by descending score (ties in ascending ord); a NaN score is in no answer, a NaN threshold throws */
  searchRange(query: Float32Array, targetVectors: BinarizedByteVectorValues, threshold: number, options?: { rowFilter?: RowFilter | null; order?: 'ord' | 'score' }): Array<{ index: number; score: number }>;
  /** extension: the same for many queries per call; one filter serves all of them */
  searchNearestNeighborsBatchFiltered(queries: Float32Array[], targetVectors: BinarizedByteVectorValues, filter: RowFilter, k: number): Array<Array<{ index: number; score: number }>>;
  /** src/binaryQuantizationFormat.ts:483-566 with the double-pack bug fixed: binaryValues is the packed row */
  serializeVectorData(vectors: Float32Array[]): { vectorData: VectorDataFormat[]; metadata: MetadataFormat };
  deserializeVectorData(vectorData: VectorDataFormat[], metadata: MetadataFormat): BinarizedByteVectorValues;
  /** extension: <prefix>.veb (device tile records) + <prefix>.vemb (MetadataFormat + centroid) */
  saveIndex(quantizedVectors: BinarizedByteVectorValues, pathPrefix: string): void;
  loadIndex(pathPrefix: string): BinarizedByteVectorValues;
  /** src/binaryQuantizationFormat.ts:420-476: every query against vector 0, quantized vs fp32 score */
  computeQuantizationAccuracy(originalVectors: Float32Array[], queryVectors: Float32Array[]): { meanError: number; maxError: number; minError: number; stdError: number; correlation: number };
  getConfig(): BinaryQuantizationConfig;
  getQuantizer(): OptimizedScalarQuantizer;
  getScorer(): BinaryQuantizedScorer;
}
export interface VectorDataFormat { binaryValues: Uint8Array; lowerInterval: number; upperInterval: number; additionalCorrection: number; quantizedComponentSum: number; }
export interface MetadataFormat { fieldNumber: number; vectorEncodingOrdinal: number; vectorSimilarityOrdinal: number; dimensions: number; vectorDataOffset: number; vectorDataLength: number; vectorCount: number; centroid: Float32Array; centroidSquareMagnitude: number; }
export interface SiftVector { dimension: number; values: Float32Array; }
export interface SiftDataset { vectors: SiftVector[]; count: number; dimension: number; }
export declare function loadSiftVectors(filePath: string, maxVectors?: number): SiftDataset;
export declare function loadSiftDataset(datasetDir: string, fileType?: 'base' | 'learn' | 'query', maxVectors?: number): SiftDataset;
export declare function loadSiftQueries(datasetDir: string, maxQueries?: number): { queries: SiftVector[]; groundtruth: number[][] };
export declare function normalizeVector(vector: Float32Array): Float32Array;
export declare function computeCentroid(vectors: Float32Array[]): Float32Array;
export declare function computeDotProduct(a: Float32Array, b: Float32Array): number;
export declare function computeEuclideanDistance(a: Float32Array, b: Float32Array): number;
export declare function computeEuclideanSimilarity(a: Float32Array, b: Float32Array): number;
export declare function computeCosineSimilarity(a: Float32Array, b: Float32Array): number;
export declare function computeMaximumInnerProduct(a: Float32Array, b: Float32Array): number;
export declare function computeSimilarity(a: Float32Array, b: Float32Array, similarityFunction: 'EUCLIDEAN' | 'COSINE' | 'MAXIMUM_INNER_PRODUCT'): number;
export declare function computeQuantizedDotProduct(q: Uint8Array, d: Uint8Array): number;
export declare function computeInt4BitDotProduct(q: Uint8Array, d: Uint8Array): number;
export declare function computeInt1BitDotProduct(q: Uint8Array, d: Uint8Array): number;
export interface TopKCandidate { index: number; quantizedScore: number; trueScore: number; }
/** the original fp32 vectors resident on the GPU; accepted wherever the selectors take `vectors` */
export declare class DeviceVectors {
  constructor(vectors: Float32Array[], device?: number);
  readonly length: number;
  readonly dim: number;
  /** computeSimilarity(query, vectors[rows[j]]) (f64, bit-identical to src/vectorSimilarity.ts); default COSINE */
  trueScores(query: Float32Array, rows: ArrayLike<number>, similarityFunction?: VectorSimilarityFunction): Float64Array;
  /** extension: the fp32 rows of a block BinaryQuantizationFormat.appendVectors has added to the index get the next ords */
  append(vectors: Float32Array[]): DeviceVectors;
  /** extension: the fp32 rows of a block BinaryQuantizationFormat.updateVectors has put into the index replace the rows `ords` */
  update(ords: Int32Array | number[], vectors: Float32Array[]): DeviceVectors;
  /** extension: the fp32 rows follow BinaryQuantizationFormat.compactVectors: the rows `filter` accepts are kept, in order, on the device */
  compact(filter: RowFilter): DeviceVectors;
  /** extension: the exact top-k of every raw query over the resident rows (those `filter` accepts), scored in f64 and selected on the device: descending, equal scores by ascending row, a NaN last (bbq_vectors_search_batch); default COSINE */
  trueTopK(queries: Float32Array[], k: number, similarityFunction?: VectorSimilarityFunction, filter?: RowFilter | null): Array<Array<{ index: number; trueScore: number }>>;
  /** extension: 'exact_slab_rows', the rows trueTopK scores between two select passes (0: automatic); never changes an answer */
  setOption(name: string, value: number): DeviceVectors;
  dispose(): void;
}
export declare function createDeviceVectors(vectors: Float32Array[], device?: number): DeviceVectors;
/** extension: an accept set of the rows of one index, resident on its device; not supported on a multi-device index (BBQ_DEVICES) */
export declare class RowFilter {
  constructor(targetVectors: BinarizedByteVectorValues, accept: Uint8Array | Int32Array | number[] | ((ord: number) => boolean));
  readonly count: number;
  dispose(): void;
}
export declare function createRowFilter(targetVectors: BinarizedByteVectorValues, accept: Uint8Array | Int32Array | number[] | ((ord: number) => boolean)): RowFilter;
/** extension: the groups of the rows of targetVectors - group g is the rows [offsets[g], offsets[g + 1]) - resident on its device; `filter` says which rows exist */
export declare class RowGroups {
  constructor(targetVectors: BinarizedByteVectorValues, offsets: number[] | Float64Array, filter?: RowFilter | null);
  /** the number of groups, empty ones included */
  readonly count: number;
  /** the groups with at least one accepted row */
  readonly live: number;
  dispose(): void;
}
export declare function createRowGroups(targetVectors: BinarizedByteVectorValues, offsets: number[] | Float64Array, filter?: RowFilter | null): RowGroups;
export declare function getOversampledTopKWithHeap(query: Float32Array, quantizedVectors: any, vectors: Float32Array[] | DeviceVectors, k: number, oversampleFactor: number, format: BinaryQuantizationFormat): TopKCandidate[];
export declare function getOversampledTopKWithSort(query: Float32Array, quantizedVectors: any, vectors: Float32Array[] | DeviceVectors, k: number, oversampleFactor: number, format: BinaryQuantizationFormat): TopKCandidate[];
/** getTrueTopK, tests/recall-common.ts:143-149: the indices of the k rows of greatest computeCosineSimilarity; with DeviceVectors every row is scored and the k best are selected on the device */
export declare function getTrueTopK(query: Float32Array, vectors: Float32Array[] | DeviceVectors, k: number): number[];
/** extension: the whole recipe for many queries in one native call */
export declare function getOversampledTopKBatch(queries: Float32Array[], quantizedVectors: any, vectors: DeviceVectors, k: number, oversampleFactor: number, format: BinaryQuantizationFormat, selector?: 'heap' | 'sort'): TopKCandidate[][];
/** extension: the exact MaxSim score of every candidate group, in list order - per token the greatest computeSimilarity among the group's accepted fp32 rows, summed in f64 in token order (bbq_rerank_maxsim_groups_batch) */
export declare function computeMaxSimGroupTrueScores(queryVectors: Float32Array[], vectors: DeviceVectors, rowGroups: RowGroups, groupNumbers: Int32Array | number[], similarity?: VectorSimilarityFunction): Float64Array;
/** extension: searchNearestNeighborsMaxSim with k * oversampleFactor, exact MaxSim scores of the returned groups, then the heap or the sort selector over them (bbq_search_maxsim_rerank_batch) */
export declare function getOversampledMaxSimTopK(queryVectors: Float32Array[], targetVectors: BinarizedByteVectorValues, vectors: DeviceVectors, rowGroups: RowGroups, k: number, oversampleFactor: number, format: BinaryQuantizationFormat, selector?: 'heap' | 'sort'): Array<{ group: number; quantizedScore: number; trueScore: number }>;
export declare const DEFAULT_CONFIG: { readonly queryBits: 4; readonly indexBits: 1; readonly quantizer: { readonly similarityFunction: VectorSimilarityFunction.COSINE; readonly lambda: 0.1; readonly iters: 5 } };
export declare function createBinaryQuantizationFormat(config?: BinaryQuantizationConfig): BinaryQuantizationFormat;
export declare function quickQuantize(vectors: Float32Array[], similarityFunction?: VectorSimilarityFunction): { quantizedVectors: BinarizedByteVectorValues; queryQuantizer: OptimizedScalarQuantizer };
export declare function quickSearch(queryVector: Float32Array, targetVectors: Float32Array[], k: number, similarityFunction?: VectorSimilarityFunction): Array<{ index: number; score: number }>;
export declare const VERSION: string;
export declare function deviceCount(): number;

// helpers and constants the reference re-exports from its root (src/index.ts:20-37)
export declare const NUMERICAL_CONSTANTS: { readonly CONVERGENCE_THRESHOLD: 1e-8; readonly MIN_DETERMINANT: 1e-12; readonly EPSILON: 1e-8 };
export declare const FILE_EXTENSIONS: { readonly VECTOR_DATA: 'veb'; readonly META: 'vemb' };
export declare const COMPONENT_NAMES: { readonly BINARIZED_VECTOR: 'BVEC' };
export declare const MINIMUM_MSE_GRID: number[][];
export declare const BIT_COUNT_LOOKUP_TABLE: Uint8Array;
export declare function computeL2Norm(vector: Float32Array): number;
export declare function computeMean(vector: Float32Array): number;
export declare function computeStd(vector: Float32Array, mean: number): number;
export declare function clamp(x: number, min: number, max: number): number;
export declare function bitCount(n: number): number;
export declare function bitCountBytes(bytes: Uint8Array): number;
export declare function bitCountBytesOptimized(bytes: Uint8Array): number;
export declare function getBitCount(byte: number): number;
export declare function isNearZero(value: number, threshold?: number): boolean;
export declare function isNearEqual(a: number, b: number, epsilon?: number): boolean;
export declare function scaleMaxInnerProductScore(score: number): number;
export declare function addVectors(a: Float32Array, b: Float32Array): Float32Array;
export declare function subtractVectors(a: Float32Array, b: Float32Array): Float32Array;
export declare function scaleVector(vector: Float32Array, scalar: number): Float32Array;
export declare function centerVector(vector: Float32Array, centroid: Float32Array): Float32Array;
export declare function copyVector(vector: Float32Array): Float32Array;
export declare function computeVectorMagnitude(vector: Float32Array): number;
export declare function createRandomVector(dimension: number, min?: number, max?: number): Float32Array;
export declare function createZeroVector(dimension: number): Float32Array;
export interface QuantizationAccuracy { meanError: number; maxError: number; minError: number; stdError: number; correlation: number; }
/** src/index.ts:120-134: computeQuantizationAccuracy of a format with lambda 0.1 / 5 iterations */
export declare function computeAccuracy(originalVectors: Float32Array[], queryVectors: Float32Array[], similarityFunction?: VectorSimilarityFunction): QuantizationAccuracy;
