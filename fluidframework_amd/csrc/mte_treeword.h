// mte_treeword.h — the tree word's accessors (the word: mte_tree.h; its bits:
// mte_passes.h) and the reference's block constants.  Included by both tree
// passes (mte_tree.h, mte_htree.h), which share nothing else.
#pragma once

#include "mte_passes.h"

namespace mte {

constexpr uint32_t kNsUndef = 0, kNsFalse = 1, kNsTrue = 2;
constexpr int kMaxNodes = 8;       // MaxNodesInBlock, mergeTreeNodes.ts:373
constexpr int32_t kTextGranularity = 256;  // textSegment.ts:19

__device__ __forceinline__ uint32_t t_h(uint32_t t) { return t & kTH; }
__device__ __forceinline__ uint32_t t_ns(uint32_t t) { return (t & kTNs) >> kTNsShift; }
__device__ __forceinline__ uint32_t t_id(uint32_t t) { return (t >> 8) & (kIdLimit - 1u); }

}  // namespace mte
