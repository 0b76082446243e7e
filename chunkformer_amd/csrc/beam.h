// What the beam searches share (ctc_beam.hip, rnnt_beam.hip, attdec.hip): the beam limit, the error word, log_add,
// the prefix trie that gives a hypothesis its identity, its workspace regions, and one round of the top-K selection.
// A search mode is its scoring kernel plus calls into these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "cfm_common.h"
#include "workspace.h"

namespace cfm {

constexpr int BEAM_KMAX = 16;   // the largest beam of every search
constexpr double NINF = -INFINITY;

// the error word (first int32 of a search's workspace; include/cfm.h documents the values)
enum {
  BEAM_ERR_RANGE = 1,   // a row range outside the rows
  BEAM_ERR_MAP = 2,     // the trie's map is full (cannot happen: at most K * len inserts into 2 * K * len slots)
  BEAM_ERR_EMPTY = 3,   // a frame left no candidate
  BEAM_ERR_NAN = 4      // a NaN score was ranked as -inf
};

CFM_DEV double log_add(double a, double b) {   // utils/common.py:201-209 log_add on [a, b]
  if (a == NINF && b == NINF) return NINF;
  const double m = a > b ? a : b;
  return m + log(0.0 + exp(a - m) + exp(b - m));
}

// ----------------------------------------------------------------------------- prefix trie
// The trie's arrays for all utterances of a call: utterance (start, len) owns K * len entries at K * start (the map:
// twice that).  Carved from a workspace on the host; with a null base the Carver only counts.
struct TrieRegions {
  int32_t *node_par, *node_tok, *map, *tprev, *tframe;
};
inline TrieRegions carve_trie(Carver& c, size_t nodes, bool with_times) {
  TrieRegions r{};
  r.node_par = c.take<int32_t>(nodes);
  r.node_tok = c.take<int32_t>(nodes);
  r.map = c.take<int32_t>(2 * nodes);
  if (with_times) {
    r.tprev = c.take<int32_t>(nodes);
    r.tframe = c.take<int32_t>(nodes);
  }
  return r;
}

CFM_DEV uint32_t edge_hash(int par, int tok) {
  uint32_t h = (uint32_t)par * 0x9E3779B1u ^ ((uint32_t)tok + 0x7F4A7C15u) * 0x85EBCA6Bu;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
  return h;
}

// One utterance's view of the regions (nothing shared between workgroups, no allocation counters):
//   trie    node id 0 = the empty prefix; node 1 + t * K + r is the prefix that survivor r of frame t created:
//           (parent node, token), at [id - 1].
//   map     open addressing, 2 * K * len slots of node ids (0 = empty), keyed by the (parent, token) of the node a
//           slot names.  It lives for the whole utterance, so a prefix has ONE node id however often it leaves and
//           re-enters the beam.  The search zeroes it before the first frame.
//   times   persistent lists: entry 1 + t * K + r = (previous entry, frame t), at [id - 1]; 0 = the empty list.  A
//           copy shares the entry id, an append makes the survivor's one entry.
struct PrefixTrie {
  int32_t *par, *tok, *map, *tprev, *tframe;
  int K, len, cap;

  CFM_DEV PrefixTrie(const TrieRegions& r, int K_, int start, int len_, bool with_times)
      : par(r.node_par + (size_t)K_ * start), tok(r.node_tok + (size_t)K_ * start),
        map(r.map + (size_t)2 * K_ * start), tprev(with_times ? r.tprev + (size_t)K_ * start : nullptr),
        tframe(with_times ? r.tframe + (size_t)K_ * start : nullptr), K(K_), len(len_), cap(2 * K_ * len_) {}

  // the node (parent, token), or 0 when the prefix has never been in the beam
  CFM_DEV int find(int parent, int token) const {
    if (cap == 0) return 0;
    int s = (int)(edge_hash(parent, token) % (uint32_t)cap);
    for (int probe = 0; probe < cap; ++probe) {
      const int v = map[s];
      if (v == 0) return 0;
      if (par[v - 1] == parent && tok[v - 1] == token) return v;
      s = s + 1 == cap ? 0 : s + 1;
    }
    return 0;
  }

  // node = (parent, token), which find() did not find; false when the map is full (the caller sets BEAM_ERR_MAP)
  CFM_DEV bool insert(int node, int parent, int token) const {
    par[node - 1] = parent;
    tok[node - 1] = token;
    int s = (int)(edge_hash(parent, token) % (uint32_t)cap), probe = 0;
    for (; probe < cap; ++probe) {
      if (atomicCAS(&map[s], 0, node) == 0) break;
      s = s + 1 == cap ? 0 : s + 1;
    }
    return probe != cap;
  }

  CFM_DEV void time_append(int entry, int prev, int frame) const {
    tprev[entry - 1] = prev;
    tframe[entry - 1] = frame;
  }

  // The finish walks.  Ids never exceed K * len and a chain holds one entry per frame at most: both are loop bounds.
  // tokens of `node`, first token first, into out[0 .. L); returns L
  CFM_DEV int tokens(int node, int32_t* out) const {
    const int top = K * len;
    int L = 0;
    for (int nd = node; nd > 0 && nd <= top && L < len; nd = par[nd - 1]) ++L;
    int i = L;
    for (int nd = node; nd > 0 && nd <= top && i > 0; nd = par[nd - 1]) out[--i] = tok[nd - 1];
    return L;
  }
  // the frames of time list `entry` into out[0 .. L), last frame last; a shorter list is padded in front with -1
  CFM_DEV void frames(int entry, int L, int32_t* out) const {
    const int top = K * len;
    int i = L;
    for (int tn = entry; tn > 0 && tn <= top && i > 0; tn = tprev[tn - 1]) out[--i] = tframe[tn - 1];
    while (i > 0) out[--i] = -1;
  }
};

// ----------------------------------------------------------------------------- top K by rounds
// The K largest of a set of (key, index) in the order (key descending, index ascending), over order-preserving keys
// (f2key): round r takes the first element that comes after round r - 1's pick in that order, so nothing is marked
// or moved.  Every lane see()s its elements, the lanes reduce, next() makes the pick the bound of the next round.
constexpr int TOPK_NONE = 0x7fffffff;   // the index of "no element"

struct TopKRound {
  uint32_t pk = 0xffffffffu, bk = 0u;   // previous pick, running best
  int pi = -1, bi = TOPK_NONE;

  // whether (key, index) comes before the running best
  CFM_DEV bool better(uint32_t key, int index) const {
    return index != TOPK_NONE && (bi == TOPK_NONE || key > bk || (key == bk && index < bi));
  }
  CFM_DEV void merge(uint32_t key, int index) {
    if (better(key, index)) { bk = key; bi = index; }
  }
  CFM_DEV void see(uint32_t key, int index) {   // index: a real one
    const bool after = key < pk || (key == pk && index > pi);
    if (after && (bi == TOPK_NONE || key > bk || (key == bk && index < bi))) { bk = key; bi = index; }
  }
  CFM_DEV void reduce64() {   // every lane ends with the wave's best
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(__shfl_xor(bk, o, 64), __shfl_xor(bi, o, 64));
  }
  CFM_DEV void next() {
    pk = bk; pi = bi;
    bk = 0u; bi = TOPK_NONE;
  }
};

}  // namespace cfm
