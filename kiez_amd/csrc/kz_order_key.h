// THE ORDER-PRESERVING 64-BIT KEY OF A DOUBLE: a double with the sign bit set has all its bits flipped, any other gets the sign bit
// set -- unsigned keys then order like the doubles, -inf first -- after NaN has taken +inf's pattern and -0.0 that of +0.0:
// kz_rank_before's rule (NaN ranks as +inf, both tie by row; -0.0 == +0.0) as one integer compare.  Shared by the whole-index
// selection (kz_knn_reduced.h) and the one-to-one matching (kz_match.hip), which both order values that can be negative, infinite
// or NaN with integer compares and integer atomics only.
#pragma once

__device__ __forceinline__ unsigned long long kz_knnr_key(double w) {
    unsigned long long b = (unsigned long long)__double_as_longlong(w);
    if (w != w) b = 0x7ff0000000000000ull;   // NaN ranks as +inf
    if (w == 0.0) b = 0ull;                  // -0.0 == +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
constexpr unsigned long long KZ_KNNR_PAD = ~0ull;   // a place without an entry: above +inf's key (0xfff0...), the largest a w has
