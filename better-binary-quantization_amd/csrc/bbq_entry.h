// bbq_entry.h - the 64-bit words the device and the host exchange: candidate / answer entries, the monotone keys thresholds are
// compared in, the header of an answer block.  Needs nothing of HIP (bbq_replay.cpp builds with a plain host compiler too).
#pragma once
#include <stdint.h>
#include <string.h>
#ifdef __HIP__
#define BBQ_HD __host__ __device__
#else
#define BBQ_HD
#endif

namespace bbq {

// an entry: global row << 32 | f32 score bits - entries of distinct rows order like their rows
BBQ_HD inline uint64_t make_entry(uint32_t row, uint32_t score_bits) { return ((uint64_t)row << 32) | score_bits; }
BBQ_HD inline uint32_t entry_row(uint64_t e) { return (uint32_t)(e >> 32); }
BBQ_HD inline uint32_t entry_bits(uint64_t e) { return (uint32_t)e; }
inline float entry_score(uint64_t e) {
  float f;
  memcpy(&f, &e, 4);  // the low word (little-endian host)
  return f;
}
// n entries as the (row, score) pairs of an answer
inline void unpack_entries(const uint64_t *e, int64_t n, int32_t *rows, float *scores) {
  for (int64_t j = 0; j < n; ++j) {
    rows[j] = (int32_t)entry_row(e[j]);
    scores[j] = entry_score(e[j]);
  }
}
// f32 score bits <-> a key that orders as unsigned like the score orders as a float
BBQ_HD inline uint32_t key_of_bits(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
BBQ_HD inline uint32_t bits_of_key(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// The header of one query's answer block (FinalizeArgs::final_out): word 0 = {entries listed | flags << 32}, word 1 = {answer entries |
// 1 = not proven, replay the list on the host << 32}, then the entries; a shard's block (final_shard) has its cut key in word 2 first.
struct AnswerHeader {
  uint32_t listed, flags, count, needs_replay;
  explicit AnswerHeader(const uint64_t *b) : listed((uint32_t)b[0]), flags((uint32_t)(b[0] >> 32)), count((uint32_t)b[1]), needs_replay((uint32_t)(b[1] >> 32)) {}
};
BBQ_HD inline uint64_t header_word(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
inline uint32_t shard_cut(const uint64_t *b) { return (uint32_t)b[2]; }

}  // namespace bbq
