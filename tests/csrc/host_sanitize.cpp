// Exercises the host-only part of libbbq (quantizer, heap replay, error plumbing: bbq_quantizer.cpp + bbq_replay.cpp, no HIP) through
// the C ABI and, for what has no entry point of its own - the proof of a selected answer block, the thread fan-out, the list-order
// replay - through bbq_internal.h; built by tests/test_sanitizers_cpu.py with -fsanitize=address,undefined and with -fsanitize=thread.  GPU sanitizers are
// not available on this pool, so this is where memory and thread errors of the host code are looked for.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/bbq.h"
#include "../../better-binary-quantization_amd/csrc/bbq_internal.h"  // the host-only internals next to HeapReplay: prove_selected, for_each_index, replay_lists

static uint32_t rng_state = 12345;
static float frand() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (float)((rng_state >> 8) & 0xFFFF) / 32768.0f - 1.0f;
}
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "check failed at line %d: %s (%s)\n", __LINE__, #cond, bbq_last_error()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main() {
  const int dims[] = {1, 7, 64, 100, 129};
  const int bits[] = {1, 2, 4, 8};
  for (int dim : dims)
    for (int ib : bits)
      for (int sim = 0; sim < 3; ++sim) {
        const int64_t n = 257;
        std::vector<float> v((size_t)n * dim);
        for (float &x : v) x = frand();
        const int64_t rb = ib == 1 ? (dim + 7) / 8 : dim;
        std::vector<uint8_t> codes((size_t)(n * rb));
        std::vector<double> corr((size_t)n * 4);
        std::vector<float> cen((size_t)dim);
        int64_t bad_row = -1;
        int32_t bad_col = -1;
        CHECK(bbq_quantize_vectors(v.data(), n, dim, sim, ib, 0.1, 5, 4, codes.data(), corr.data(), cen.data(), &bad_row, &bad_col) == BBQ_OK);
        if (ib > 1)
          for (uint8_t c : codes) CHECK(c < (1u << ib));
        // queries: one by one and as a batch on threads, identical
        const int nq = 9;
        std::vector<float> q((size_t)nq * dim);
        for (float &x : q) x = frand();
        std::vector<uint8_t> qq((size_t)nq * dim), qq1((size_t)dim);
        std::vector<double> qc((size_t)nq * 4), qc1(4);
        int32_t bad_q = -1;
        CHECK(bbq_quantize_queries(q.data(), nq, dim, cen.data(), sim, 4, 0.1, 5, 3, qq.data(), qc.data(), &bad_q) == BBQ_OK);
        for (int i = 0; i < nq; ++i) {
          CHECK(bbq_quantize_query(q.data() + (size_t)i * dim, dim, cen.data(), sim, 4, 0.1, 5, qq1.data(), qc1.data()) == BBQ_OK);
          CHECK(memcmp(qq1.data(), qq.data() + (size_t)i * dim, (size_t)dim) == 0);
          CHECK(memcmp(qc1.data(), qc.data() + (size_t)i * 4, 32) == 0);
        }
        (void)bbq_centroid_dp(cen.data(), dim);
      }
  {  // the reference's input errors
    std::vector<float> v = {1.f, NAN, 3.f, 4.f};
    std::vector<uint8_t> codes(8);
    std::vector<double> corr(8);
    std::vector<float> cen(2);
    int64_t bad_row = -1;
    int32_t bad_col = -1;
    CHECK(bbq_quantize_vectors(v.data(), 2, 2, 0, 1, 0.1, 5, 2, codes.data(), corr.data(), cen.data(), &bad_row, &bad_col) == BBQ_ERR_NAN_INPUT);
    CHECK(bad_row == 0 && bad_col == 1);
    CHECK(bbq_quantize_vectors(v.data(), 0, 2, 0, 1, 0.1, 5, 2, codes.data(), corr.data(), cen.data(), nullptr, nullptr) == BBQ_ERR_EMPTY);
    CHECK(strlen(bbq_last_error()) > 0);
  }
  {  // heap replay: several sources, many queries, host threads; ties; k = 0, k > rows
    const int S = 3, Q = 50;
    const int64_t per = 400, n_total = S * per;
    std::vector<std::vector<bbq_cand>> packed((size_t)S);
    std::vector<std::vector<int64_t>> offsets((size_t)S);
    for (int s = 0; s < S; ++s) {
      offsets[(size_t)s].push_back(0);
      for (int qi = 0; qi < Q; ++qi) {
        for (int64_t r = 0; r < per; ++r) {
          if (((r * 7 + qi) % 3) == 0) continue;  // ragged lists
          const float sc = (float)((r * 31 + qi * 17 + s) % 23) * 0.125f;  // few distinct scores: ties everywhere
          uint32_t b;
          memcpy(&b, &sc, 4);
          packed[(size_t)s].push_back(((uint64_t)(uint32_t)(s * per + r) << 32) | b);
        }
        offsets[(size_t)s].push_back((int64_t)packed[(size_t)s].size());
      }
    }
    const bbq_cand *pp[S];
    const int64_t *po[S];
    for (int s = 0; s < S; ++s) { pp[s] = packed[(size_t)s].data(); po[s] = offsets[(size_t)s].data(); }
    for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)37, (int64_t)5000}) {
      std::vector<int32_t> idx((size_t)(Q * (k > 0 ? k : 1))), idx1((size_t)(k > 0 ? k : 1));
      std::vector<float> sc((size_t)(Q * (k > 0 ? k : 1))), sc1((size_t)(k > 0 ? k : 1));
      std::vector<int64_t> cnt((size_t)Q);
      CHECK(bbq_replay_batch(S, pp, po, Q, n_total, k, 4, idx.data(), sc.data(), cnt.data()) == BBQ_OK);
      for (int qi = 0; qi < Q; qi += 7) {  // the single-query entry point agrees
        const bbq_cand *l[S];
        int64_t c[S];
        for (int s = 0; s < S; ++s) { l[s] = pp[s] + po[s][qi]; c[s] = po[s][qi + 1] - po[s][qi]; }
        int64_t n1 = -1;
        CHECK(bbq_replay(S, l, c, n_total, k, idx1.data(), sc1.data(), &n1) == BBQ_OK);
        CHECK(n1 == cnt[(size_t)qi]);
        CHECK(k == 0 || memcmp(idx1.data(), idx.data() + (size_t)qi * k, (size_t)n1 * 4) == 0);
      }
    }
    int64_t n1 = 0;
    CHECK(bbq_replay(1, pp, nullptr, n_total, 5, nullptr, nullptr, &n1) == BBQ_ERR_INVALID_ARG);
    CHECK(bbq_replay_batch(S, pp, po, Q, n_total, -1, 2, nullptr, nullptr, nullptr) != BBQ_OK);
  }
  {  // the proof of one answer block of the select pass: {above the cut | NaN seen << 32}, the cut, then the entries
    auto entry = [](uint32_t row, float score) {
      uint32_t b;
      memcpy(&b, &score, 4);
      return ((uint64_t)row << 32) | b;
    };
    auto block = [&](uint32_t count, uint32_t nan_seen, float cut, std::vector<float> scores) {
      std::vector<uint64_t> blk = {(uint64_t)count | ((uint64_t)nan_seen << 32), entry(0, cut)};
      for (size_t i = 0; i < scores.size(); ++i) blk.push_back(entry(100 + (uint32_t)i, scores[i]));
      return blk;
    };
    std::vector<uint64_t> ent;
    int32_t rows[4];
    float sc[4];
    const std::vector<uint64_t> clean = block(4, 0, 0.5f, {2.f, 9.f, 1.f, 4.f});  // k distinct scores above the cut, unsorted
    CHECK(bbq::prove_selected(clean.data(), 4, ent) && ent.size() == 4);
    bbq::unpack_entries(ent.data(), 4, rows, sc);
    CHECK(rows[0] == 101 && rows[1] == 103 && rows[2] == 100 && rows[3] == 102);
    CHECK(sc[0] == 9.f && sc[1] == 4.f && sc[2] == 2.f && sc[3] == 1.f);
    CHECK(!bbq::prove_selected(block(4, 1, 0.5f, {2.f, 9.f, 1.f, 4.f}).data(), 4, ent));  // the NaN word
    CHECK(!bbq::prove_selected(block(3, 0, 0.5f, {2.f, 9.f, 1.f, 4.f}).data(), 4, ent));  // a count other than k: fewer ...
    CHECK(!bbq::prove_selected(block(5, 0, 0.5f, {2.f, 9.f, 1.f, 4.f}).data(), 4, ent));  // ... and more
    CHECK(!bbq::prove_selected(block(4, 0, 0.5f, {2.f, 9.f, 2.f, 4.f}).data(), 4, ent));  // two equal neighbours once sorted
    CHECK(!bbq::prove_selected(block(4, 0, 0.f, {2.f, 9.f, -0.f, 4.f}).data(), 4, ent));  // the k-th equals the cut (+0.0 == -0.0)
    CHECK(!bbq::prove_selected(block(4, 0, 1.f, {2.f, 9.f, 1.f, 4.f}).data(), 4, ent));   // the same, bit for bit
    const std::vector<uint64_t> one = block(1, 0, 3.f, {7.f});  // k = 1
    CHECK(bbq::prove_selected(one.data(), 1, ent) && ent.size() == 1);
    bbq::unpack_entries(ent.data(), 1, rows, sc);
    CHECK(rows[0] == 100 && sc[0] == 7.f);
    CHECK(!bbq::prove_selected(block(1, 0, 7.f, {7.f}).data(), 1, ent));
  }
  {  // the fan-out: every index exactly once, whatever the thread count - one thread, four, more threads than indices, none
    for (int T : {1, 4, 0})
      for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)1000}) {  // n = 3 < T = 4
        std::vector<int> hits((size_t)n, 0);
        bbq::for_each_index(T, n, [&](int64_t i) { ++hits[(size_t)i]; });
        for (int h : hits) CHECK(h == 1);
      }
  }
  {  // the list-order replay: on one thread and on four, below and above its thread threshold, the same answers as bbq_replay's heap
    const int Q = 9;
    const int64_t k = 5;
    for (int64_t len : {(int64_t)7, (int64_t)700}) {
      std::vector<int64_t> off = {0};
      std::vector<int32_t> tags;
      std::vector<float> scores;
      for (int q = 0; q < Q; ++q) {
        for (int64_t i = 0; i < (q == 4 ? 0 : len + q); ++i) {  // list 4 is empty
          tags.push_back((int32_t)((i * 37 + q) % 1000));   // not ascending: the order given is the order offered
          scores.push_back((float)((i * 31 + q * 17) % 23) * 0.125f);
        }
        off.push_back((int64_t)tags.size());
      }
      std::vector<int32_t> t1((size_t)(Q * k), -1), t4((size_t)(Q * k), -1);
      std::vector<float> s1((size_t)(Q * k), -1.f), s4((size_t)(Q * k), -1.f);
      std::vector<int64_t> n1((size_t)Q, -1), n4((size_t)Q, -1);
      bbq::replay_lists(Q, off.data(), tags.data(), scores.data(), k, 1, t1.data(), s1.data(), n1.data());
      bbq::replay_lists(Q, off.data(), tags.data(), scores.data(), k, 4, t4.data(), s4.data(), n4.data());
      CHECK(t1 == t4 && s1 == s4 && n1 == n4 && n1[4] == 0 && n1[0] == k);
      for (int q = 0; q < Q; ++q) {
        bbq::HeapReplay hr(k, off[(size_t)q + 1] - off[(size_t)q]);
        for (int64_t i = off[(size_t)q]; i < off[(size_t)q + 1]; ++i) hr.offer(scores[(size_t)i], tags[(size_t)i]);
        int32_t ht[5];
        float hs[5];
        CHECK(hr.finish(ht, hs) == n1[(size_t)q]);
        CHECK(memcmp(ht, t1.data() + q * k, (size_t)n1[(size_t)q] * 4) == 0 && memcmp(hs, s1.data() + q * k, (size_t)n1[(size_t)q] * 4) == 0);
      }
      std::vector<int64_t> n0((size_t)Q, -1);
      bbq::replay_lists(Q, off.data(), tags.data(), scores.data(), 0, 4, nullptr, nullptr, n0.data());  // k = 0 answers nothing
      for (int64_t c : n0) CHECK(c == 0);
    }
  }
  printf("host sanitize ok\n");
  return 0;
}
