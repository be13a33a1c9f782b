// str_minmax.h — MIN / MAX over VARCHAR as rounds of 64-bit atomicMin /
// atomicMax (str_kernels.hip: str_minmax_key, _live, _round, _rows; the
// executor's side is StrMinMaxColumns in aggregate.cpp).
//
// Every group has one 64-bit word per kind (MIN, MAX) and round.  In a round
// every live row offers a key to its group's word; when the round is over, a
// row stays live only if its key equals the word.  The rounds of a run with C
// chunks are
//
//   r = 0 .. C-1   chunk r of the string: its bytes [8r, 8r+8) big-endian,
//                  zero-padded (the key sort_key_str_kernel builds); MIN takes
//                  the least, MAX the greatest
//   r = C          the string's length: live rows of a group now agree on
//                  every byte up to 8C and so differ in trailing NUL bytes at
//                  most; the shorter is the smaller (StrCompare)
//   r = C + 1      the row number, least first for both kinds: equal strings
//
// A word starts at the value no key can improve on from the wrong side (all
// ones where the round takes the least, 0 where it takes the greatest), and a
// row is live when its key *equals* the word, not when it changed it: a group
// of '' only offers key 0 to a MAX word that is 0 already and still wins.
// After round C + 1 the word is the winner's row number, or still all ones for
// a group without a non-NULL row.
//
// Chunk 0 orders most rows for good: comparing the zero-padded first 8 bytes
// as one big-endian number is comparing them byte by byte, unsigned, so a
// smaller key means a smaller string and only rows that tie on it go on.
// No HIP types: the functions also build in a plain host program
// (tests/plan_harness/str_minmax.cpp), which runs the same rounds in one thread.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_MM_HD __host__ __device__ __forceinline__
#else
#define MBX_MM_HD inline
#endif

namespace mbx {

enum StrMinMaxKind : int { SMM_MIN = 0, SMM_MAX = 1, SMM_KINDS = 2 };
// which kinds a run computes, as a mask
constexpr int kStrMinMaxWantMin = 1, kStrMinMaxWantMax = 2;
constexpr uint64_t kStrMinMaxNoRow = ~0ull;  // the last round's word of a group without a winner

// chunks that cover maxlen bytes (at least one: '' has a chunk, all zero)
MBX_MM_HD int StrMinMaxChunks(int64_t maxlen) { return maxlen <= 8 ? 1 : (int)((maxlen + 7) / 8); }
// rounds of a run over C chunks: the chunks, the length tie, the row tie
MBX_MM_HD int StrMinMaxRounds(int chunks) { return chunks + 2; }

// Chunk c of s[0, len): `avail` bytes may be read at s (len <= avail; the
// kernels pass what is left of the character buffer), so a whole chunk is one
// 8-byte load where 8 bytes lie in the buffer, whatever follows the string.
MBX_MM_HD uint64_t StrMinMaxChunkKey(const uint8_t *s, int64_t len, int64_t avail, int c) {
  const int64_t at = (int64_t)c * 8;
  const int64_t have = len - at;  // bytes of the string in this chunk, if > 0
  if (have <= 0) return 0;
  if (at + 8 <= avail) {
    uint64_t v;
    __builtin_memcpy(&v, s + at, 8);
    v = __builtin_bswap64(v);  // (little-endian hosts and devices only, as everything here)
    return have >= 8 ? v : v & (~0ull << (8 * (8 - have)));
  }
  uint64_t k = 0;
  for (int j = 0; j < 8; j++) k = (k << 8) | (j < have ? (uint64_t)s[at + j] : 0ull);
  return k;
}

// whether `kind`'s word takes the least key in round r of a run over C chunks
MBX_MM_HD bool StrMinMaxTakesLeast(int kind, int r, int chunks) { return kind == SMM_MIN || r == chunks + 1; }

MBX_MM_HD uint64_t StrMinMaxInitWord(int kind, int r, int chunks) {
  return StrMinMaxTakesLeast(kind, r, chunks) ? ~0ull : 0ull;
}

// the key of round r (the tie keys: the length, then the row number)
MBX_MM_HD uint64_t StrMinMaxKey(int r, int chunks, const uint8_t *s, int64_t len, int64_t avail, int64_t row) {
  if (r < chunks) return StrMinMaxChunkKey(s, len, avail, r);
  return r == chunks ? (uint64_t)len : (uint64_t)row;
}

// Whether offering `key` would change `word`.  The kernels test a plain load
// of the word with it before they issue the atomic: a word only ever moves
// towards better keys, so a stale value can cost an atomic, never lose a key.
MBX_MM_HD bool StrMinMaxImproves(bool least, uint64_t key, uint64_t word) { return least ? key < word : key > word; }
// the word after the offer (what atomicMin / atomicMax leave)
MBX_MM_HD uint64_t StrMinMaxOffer(bool least, uint64_t key, uint64_t word) {
  return StrMinMaxImproves(least, key, word) ? key : word;
}
// after the round: the row goes on only if its key is the group's
MBX_MM_HD bool StrMinMaxStaysLive(uint64_t key, uint64_t word) { return key == word; }

// A candidate: a row that was live after round 0 for at least one kind.  The
// row number and, above it, one live bit per kind.
constexpr int kStrMinMaxLiveShift = 62;
constexpr uint64_t kStrMinMaxRowMask = (1ull << kStrMinMaxLiveShift) - 1;
MBX_MM_HD uint64_t StrMinMaxCand(int64_t row, int live) { return (uint64_t)row | ((uint64_t)live << kStrMinMaxLiveShift); }
MBX_MM_HD int64_t StrMinMaxCandRow(uint64_t c) { return (int64_t)(c & kStrMinMaxRowMask); }
MBX_MM_HD int StrMinMaxCandLive(uint64_t c) { return (int)(c >> kStrMinMaxLiveShift); }

}  // namespace mbx
