// aidfp_hotword.h -- how K1 (stft.hip) reduces the 16 wave-wide ballots of a power row to the row's hot word
// (aidfp_layout.h hot_bit). No HIP in here: the two scalar primitives come in as a parameter, so
// tests/test_k1_hotword_host.py runs the same composition with the portable restatement below (plain g++).
//
// Ops::quadmask(m) is s_quadmask_b64: bit j of the result = some bit of the nibble 4j .. 4j+3 of m is set.
// Ops::pack16(lo, hi) is s_pack_ll_b32_b16: (lo & 0xFFFF) | hi << 16.
// Ops::pair(lo, hi) is lo | hi << 32 as one 64-bit register pair (no instruction: it only tells hipcc to go on in
// 64-bit operations where it would otherwise work on the two halves separately, at twice the slots).
//
// Register i < 8 of the real split holds, in lane l, the direct bin 64 i + l and the mirror bin 1024 - 64 i - l.
//   direct: lanes 16 g .. 16 g + 15 are chunk 4 i + g                      -> bit 4 i + g
//   mirror: lanes 16 g + 1 .. 16 g + 16 are chunk 63 - 4 i - g             -> bit 32 + 4 i + g
//           where "lane 64" is lane 0 of register i + 1 (bin 1024 - 64 (i + 1)); lane 0 of register 0 is the
//           dropped Nyquist bin and never counts.
// Level 1 takes one quad mask per ballot (64 lanes -> 16 quads; the mirror ballots shifted down one lane first).
// Four 16-bit results packed into one 64-bit word are four registers' quads side by side, so ONE second quad mask
// gives their 16 chunk bits in the word's order: 2 + 1/4 quad masks per ballot where the per-register form
// (two quad masks, a shift and an OR each) took 4 slots and more. The mirror registers' lane-0 bits go in at the
// packed level too: lane 0 of register i + 1 is quad bit 15 of register i.
#pragma once
#include <stdint.h>

namespace aid {

struct HotOpsPortable {  // what the two instructions compute, for hosts and tests
    static uint64_t quadmask(uint64_t m) {
        uint64_t r = 0;
        for (int j = 0; j < 16; ++j) r |= (uint64_t)(((m >> (4 * j)) & 0xFull) != 0) << j;
        return r;
    }
    static uint32_t pack16(uint32_t lo, uint32_t hi) { return (lo & 0xFFFFu) | (hi << 16); }
    static uint64_t pair(uint32_t lo, uint32_t hi) { return (uint64_t)lo | (uint64_t)hi << 32; }
};

template <class Ops>
__host__ __device__ inline uint32_t hot_quads(uint64_t ballot) {  // level 1, direct register
    return (uint32_t)Ops::quadmask(ballot);
}
template <class Ops>
__host__ __device__ inline uint32_t hot_quads_mirror(uint64_t ballot) {  // level 1, mirror register (without "lane 64")
    return (uint32_t)Ops::quadmask(ballot >> 1);
}

// two registers' level-1 words side by side (register 2 j below register 2 j + 1)
template <class Ops>
__host__ __device__ inline uint32_t hot_pair(uint32_t q_even, uint32_t q_odd) {
    return Ops::pack16(q_even, q_odd);
}

// 16 chunk bits of four registers from their two pairs; lane0 = bit 16 j set when "lane 64" of register j is hot
// (mirror registers; 0 for direct ones)
template <class Ops>
__host__ __device__ inline uint32_t hot_chunks4(uint32_t p01, uint32_t p23, uint64_t lane0) {
    return (uint32_t)Ops::quadmask(Ops::pair(p01, p23) | lane0 << 15);
}

// pd[j], pm[j]: hot_pair of direct / mirror registers 2 j, 2 j + 1; m0[i]: the low dword of mirror ballot i (bit 0 =
// its lane 0; the other bits are ignored), and m0[8] that of bin 512's ballot (every lane holds that bin): bin 512 is
// "lane 0 of register 8", the bin that closes register 7's last chunk (chunk 32, bit 63).
template <class Ops>
__host__ __device__ inline uint64_t hot_word(const uint32_t (&pd)[4], const uint32_t (&pm)[4], const uint32_t (&m0)[9]) {
    constexpr uint64_t kLane0 = 0x0001000100010001ull;
    const uint32_t lo = Ops::pack16(hot_chunks4<Ops>(pd[0], pd[1], 0), hot_chunks4<Ops>(pd[2], pd[3], 0));
    // lane 0 of registers 1..4 closes registers 0..3, lane 0 of 5..8 closes 4..7
    const uint64_t la = Ops::pair(Ops::pack16(m0[1], m0[2]), Ops::pack16(m0[3], m0[4])) & kLane0;
    const uint64_t lb = Ops::pair(Ops::pack16(m0[5], m0[6]), Ops::pack16(m0[7], m0[8])) & kLane0;
    const uint32_t hi = Ops::pack16(hot_chunks4<Ops>(pm[0], pm[1], la), hot_chunks4<Ops>(pm[2], pm[3], lb));
    return Ops::pair(lo, hi);
}

// Which of K1's 16 power stores a hot word asks for: bit 1 + i, i < 8 = direct store i (chunks 4 i .. 4 i + 3, word bits
// 4 i .. 4 i + 3), bit 9 + i = mirror store i (chunks 60 - 4 i .. 63 - 4 i, bits 32 + 4 i .. 35 + 4 i, and by its lane 0
// chunk 64 - 4 i, bit 31 + 4 i, for i > 0). ORing the upper half with itself shifted up one bit moves bit 31 + 4 i
// into nibble i, so one quad mask of the pair tests all 16 windows. (Bits 1 .. 16, not 0 .. 15: hipcc tests bit 0 of
// a word through a 64-bit lane mask, four slots where every other bit takes a bit compare and a branch.)
template <class Ops>
__host__ __device__ inline uint32_t hot_stores(uint64_t hot) {
    return (uint32_t)Ops::quadmask(hot | hot >> 32 << 33) << 1;
}

// The per-register form this replaces (two quad masks per ballot), kept as the test's reference
template <class Ops>
__host__ __device__ inline uint64_t hot_word_per_register(const uint64_t (&d)[8], const uint64_t (&m)[9]) {
    uint64_t w = 0;
    for (int i = 0; i < 8; ++i) {  // m[8]: bin 512's ballot
        w |= Ops::quadmask(Ops::quadmask(d[i])) << (4 * i);
        w |= Ops::quadmask(Ops::quadmask(m[i] >> 1)) << (32 + 4 * i);
        if (i > 0) w |= (m[i] & 1ull) << (31 + 4 * i);
    }
    return w | (m[8] & 1ull) << 63;
}

}  // namespace aid
