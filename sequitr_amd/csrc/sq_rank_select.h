// Rank selection in registers for the small-window rank filter of sq_frame_clean.hip: the element of 0-based rank R
// (ascending) of N floats, by min / max only, so the result is one of the inputs bit for bit (no NaN among them).
// Plain C++ with constant indices throughout: it compiles for the device and, for its test, for the host.
#pragma once

#if defined(__HIPCC__)
#define SQ_RS_FN __host__ __device__ __forceinline__
#else
#define SQ_RS_FN inline
#endif

SQ_RS_FN void sq_rs_sort2(float &a, float &b) {
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// "Forgetful" selection.  With L elements still to be found below the target and U above it, the largest of any
// L + 2 elements has L + 1 elements at or below it and cannot be the target, and the smallest of any U + 2 likewise:
// a working set of max(L, U) + 2 elements loses its minimum and its maximum, takes in the next element, and so on
// until one element is left.
template <int N, int R>
SQ_RS_FN float sq_rank_select(const float (&e)[N]) {
    static_assert(R >= 0 && R < N, "rank out of range");
    constexpr int L0 = R, U0 = N - 1 - R;
    constexpr int S = (L0 > U0 ? L0 : U0) + 2 < N ? (L0 > U0 ? L0 : U0) + 2 : N;
    float w[S];
#pragma unroll
    for (int i = 0; i < S; ++i) w[i] = e[i];
    int L = L0, U = U0, lo = 0, hi = S - 1, next = S;           // the working set is w[lo .. hi]
#pragma unroll
    for (int round = 0; round < N; ++round) {                   // every round drops at least one element
        if (hi > lo) {
            const int s = hi - lo + 1;
            const bool drop_max = U > 0 && s >= L + 2, drop_min = L > 0 && s >= U + 2;
            if (drop_max) {
#pragma unroll
                for (int i = 0; i < S - 1; ++i)
                    if (i >= lo && i < hi) sq_rs_sort2(w[i], w[i + 1]);
            }
            if (drop_min) {
#pragma unroll
                for (int i = S - 1; i > 0; --i)
                    if (i > lo && i <= hi - (drop_max ? 1 : 0)) sq_rs_sort2(w[i - 1], w[i]);
            }
            if (drop_min) {
                ++lo;
                --L;
            }
            if (drop_max) {
                --U;
                if (next < N) w[hi] = e[next++];
                else --hi;
            }
        }
    }
    return w[lo];
}

// The median of nine in 19 exchanges (the classic network of Paeth / Devillard for 3 x 3 median filters).
template <>
SQ_RS_FN float sq_rank_select<9, 4>(const float (&e)[9]) {
    float p0 = e[0], p1 = e[1], p2 = e[2], p3 = e[3], p4 = e[4], p5 = e[5], p6 = e[6], p7 = e[7], p8 = e[8];
    sq_rs_sort2(p1, p2); sq_rs_sort2(p4, p5); sq_rs_sort2(p7, p8);
    sq_rs_sort2(p0, p1); sq_rs_sort2(p3, p4); sq_rs_sort2(p6, p7);
    sq_rs_sort2(p1, p2); sq_rs_sort2(p4, p5); sq_rs_sort2(p7, p8);
    sq_rs_sort2(p0, p3); sq_rs_sort2(p5, p8); sq_rs_sort2(p4, p7);
    sq_rs_sort2(p3, p6); sq_rs_sort2(p1, p4); sq_rs_sort2(p2, p5);
    sq_rs_sort2(p4, p7); sq_rs_sort2(p4, p2); sq_rs_sort2(p6, p4);
    sq_rs_sort2(p4, p2);
    return p4;
}
