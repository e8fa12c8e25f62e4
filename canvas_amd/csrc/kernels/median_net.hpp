// median_net.hpp -- the two selection networks of median_ops.hip as lists of compare-exchanges.  CE(a, b) leaves the smaller of
// v[a], v[b] in v[a] and the larger in v[b]; after the list v[4] of 9, or v[12] of 25, holds the median.  Every index is a
// literal, so the values stay in registers.  Both lists are the long-published ones (J. L. Smith's 19 exchanges for 9 inputs,
// the 99 exchanges for 25 of N. Devillard's "Fast median search" collection); tests/test_median_cpu.py reads the pairs out of
// this file and proves each list on all 2^9 / 2^25 inputs of zeros and ones, which by the 0-1 principle proves it on every input.
#pragma once

#define MEDIAN_NET_9(CE) \
    CE(1, 2) CE(4, 5) CE(7, 8) CE(0, 1) CE(3, 4) CE(6, 7) CE(1, 2) CE(4, 5) CE(7, 8) CE(0, 3) \
    CE(5, 8) CE(4, 7) CE(3, 6) CE(1, 4) CE(2, 5) CE(4, 7) CE(4, 2) CE(6, 4) CE(4, 2)

#define MEDIAN_NET_25(CE) \
    CE(0, 1) CE(3, 4) CE(2, 4) CE(2, 3) CE(6, 7) CE(5, 7) CE(5, 6) CE(9, 10) CE(8, 10) CE(8, 9) CE(12, 13) \
    CE(11, 13) CE(11, 12) CE(15, 16) CE(14, 16) CE(14, 15) CE(18, 19) CE(17, 19) CE(17, 18) CE(21, 22) CE(20, 22) \
    CE(20, 21) CE(23, 24) CE(2, 5) CE(3, 6) CE(0, 6) CE(0, 3) CE(4, 7) CE(1, 7) CE(1, 4) CE(11, 14) CE(8, 14) \
    CE(8, 11) CE(12, 15) CE(9, 15) CE(9, 12) CE(13, 16) CE(10, 16) CE(10, 13) CE(20, 23) CE(17, 23) CE(17, 20) \
    CE(21, 24) CE(18, 24) CE(18, 21) CE(19, 22) CE(8, 17) CE(9, 18) CE(0, 18) CE(0, 9) CE(10, 19) CE(1, 19) \
    CE(1, 10) CE(11, 20) CE(2, 20) CE(2, 11) CE(12, 21) CE(3, 21) CE(3, 12) CE(13, 22) CE(4, 22) CE(4, 13) \
    CE(14, 23) CE(5, 23) CE(5, 14) CE(15, 24) CE(6, 24) CE(6, 15) CE(7, 16) CE(7, 19) CE(13, 21) CE(15, 23) \
    CE(7, 13) CE(7, 15) CE(1, 9) CE(3, 11) CE(5, 17) CE(11, 17) CE(9, 17) CE(4, 10) CE(6, 12) CE(7, 14) CE(4, 6) \
    CE(4, 7) CE(12, 14) CE(10, 14) CE(6, 7) CE(10, 12) CE(6, 10) CE(6, 17) CE(12, 17) CE(7, 17) CE(7, 10) \
    CE(12, 18) CE(7, 12) CE(10, 18) CE(12, 20) CE(10, 20) CE(10, 12)
