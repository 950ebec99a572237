// qattn_varlen_tile.h -- the block -> (sequence, tile) map of the packed variable-length units (qattn_varlen.hip, qattn_varlen_smooth.hip).
//
// Block -> sequence without a scan: with R rows per tile, f(i) = i + floor(start_i / R) is strictly increasing over the sequences of a
// consistent table and f(i + 1) - f(i) >= ceil(L_i / R), so workgroup j belongs to the largest i with f(i) <= j (binary search over the
// table) as its tile j - f(i) -- or to no tile, and exits.  B + ceil(total / R) workgroups per head cover every tile and waste at most B.
#pragma once
#include "qattn_common.h"

namespace qattn {

constexpr int kVarlenAmaxRows = 256;   // rows per tile of the abs-max pass
constexpr int kVarlenQuantRows = 64;   // rows per tile of the quantise pass (= one KFRAG chunk)

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

// one tile of a packed tensor: sequence i, its clamped first token and length, and the tile index within it (valid: 0 <= tile, tile R < len)
struct VarlenTile {
    int i, start, len, tile;
};
template <int R>
__device__ __forceinline__ VarlenTile varlen_tile(const int* cu, const int* used, int B, int total, int j) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {   // (workgroup-uniform) the largest i with i + floor(start_i / R) <= j
        const int mid = (lo + hi + 1) >> 1;
        const int s = clampi(__builtin_amdgcn_readfirstlane(cu[mid]), 0, total);
        if (mid + s / R <= j) lo = mid;
        else hi = mid - 1;
    }
    VarlenTile t;
    t.i = lo;
    t.start = clampi(__builtin_amdgcn_readfirstlane(cu[lo]), 0, total);
    const int end = clampi(__builtin_amdgcn_readfirstlane(cu[lo + 1]), t.start, total);
    t.len = end - t.start;
    if (used) t.len = clampi(__builtin_amdgcn_readfirstlane(used[lo]), 0, t.len);
    t.tile = j - (lo + t.start / R);
    return t;
}

}  // namespace qattn
