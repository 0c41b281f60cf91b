// ia_k3p_lds.h — the LDS formats of the split-f16 scans (ia_k3h.hip), defined once for the
// kernels, which take every pointer from them, and for the launchers (ia_k3p_launch.hip), which
// size the dynamic LDS and test what fits from them.  Host and device code include this file.
#pragma once
#include "ia_internal.h"
#include "ia_top2.h"

// how the pruned scan (k3h_prune3) streams the DB tiles it needs
enum class K3pStream {
  Whole,    // k3p_variant 20 / 21: whole tiles in two register buffers, corrections fused on query-tile pairs
  HiOnly,   // 22: the hi halves only; the lo halves of a filter-passing tile follow one tile later
  TwoPass,  // 24 / 25: a hi stream by LDS-DMA, three tiles deep, then the passing tiles whole
};

// option "k3p_variant" names a (front end, stream form) pair: 20 / 22 / 24 sort the step's queries
// in the kernel, 21 / 25 take them presorted
__host__ __device__ constexpr bool k3p_variant_pre(int v) { return v == 21 || v == 25; }
__host__ __device__ constexpr K3pStream k3p_variant_form(int v) {
  return v >= 24 ? K3pStream::TwoPass : v == 22 ? K3pStream::HiOnly : K3pStream::Whole;
}

#define IA_K3P_KS 4        // the pruned scan is 1-channel only
#define IA_K3P3_MAXQ 512   // queries of a step the in-kernel sort holds (one per thread)
#define IA_HSLOT 224  // h16x8 per slot of the two-pass form's LDS-DMA rings (3.5 KiB)
static_assert(3 * 1024 + 512 == IA_HSLOT * 16, "a slot holds pieces 0, 2, 4 (1 KiB each) and the compact piece 6");

constexpr int K3H_NW = IA_WGH / IA_WAVE;  // waves per workgroup of every split-f16 scan

// ---- k3h_scan: the query fragments [QT][2 KS][64], later overlaid by the subset merge's
// [NW][QT][32] Top2
__host__ __device__ constexpr size_t k3h_frag_bytes(int KS, int QT) { return (size_t)QT * 2 * KS * IA_WAVE * sizeof(h16x8); }
__host__ __device__ constexpr size_t k3h_red_bytes(int QT) { return (size_t)K3H_NW * QT * IA_TILE * sizeof(Top2); }
__host__ __device__ constexpr size_t k3h_lds_bytes(int KS, int QT) {
  return k3h_frag_bytes(KS, QT) > k3h_red_bytes(QT) ? k3h_frag_bytes(KS, QT) : k3h_red_bytes(QT);
}

// ---- k3h_prune3: byte offsets of its dynamic LDS.  QT query tiles (NQ = 32 QT sorted query
// slots) of a step of Mpad queries, K DB tiles per workgroup; pre: the queries arrive presorted
// (no sort arrays, skey holds the slice's slot -> query).
struct K3pLds {
  unsigned frag;    // h16x8 [QT][QFP][64] sorted query fragments (QFP = 2 KS; two passes: the KS hi pieces)
  unsigned qlo;     // float4 [NQ] projection interval lo per sorted slot
  unsigned qhi;     // float4 [NQ]                     hi
  unsigned qU;      // float [NQ] bound U'
  unsigned tlo;     // float4 [QT] query-tile boxes
  unsigned thi;     // float4 [QT]
  unsigned tU;      // float [QT], padded to a multiple of 4
  unsigned skey;    // unsigned [Mpad] sort keys   (pre: [NQ] slot -> query of the slice)
  unsigned order;   // int [Mpad] sorted -> query  (pre: none)
  unsigned rankof;  // int [Mpad] query -> sorted  (pre: none)
  unsigned wbox;    // float4 [2 K] the workgroup's tile boxes
  // 8 K bytes nobody reads or writes (once a need mask and a tile list).  Dropping them moves the
  // two-pass form's "fits 160 KiB" threshold (k3p_two_pass_fits), i.e. which launches take it: a
  // tuning change for a pull request of its own.
  unsigned unused;
  unsigned qzt;     // float [NQ] z per sorted slot (the hi x hi filter's bound)
  unsigned qzw;     // float [NQ] w per sorted slot
  unsigned wR;      // float [K] R_t of the workgroup's tiles
  unsigned plk;     // two passes: int [K] filter-passing tiles ...
  unsigned plm;     // ... unsigned [K] and their passing blocks
  unsigned end;
};
__host__ __device__ constexpr K3pLds k3p_lds(int QT, bool pre, K3pStream form, int Mpad, int K) {
  const unsigned NQ = (unsigned)QT * IA_TILE, qfp = form == K3pStream::TwoPass ? IA_K3P_KS : 2 * IA_K3P_KS;
  const unsigned nsort = pre ? 0u : (unsigned)Mpad;
  K3pLds l{};
  l.frag = 0;
  l.qlo = l.frag + (unsigned)QT * qfp * IA_WAVE * (unsigned)sizeof(h16x8);
  l.qhi = l.qlo + NQ * 16;
  l.qU = l.qhi + NQ * 16;
  l.tlo = l.qU + NQ * 4;
  l.thi = l.tlo + (unsigned)QT * 16;
  l.tU = l.thi + (unsigned)QT * 16;
  l.skey = l.tU + (((unsigned)QT + 3) & ~3u) * 4;
  l.order = l.skey + (pre ? NQ : (unsigned)Mpad) * 4;
  l.rankof = l.order + nsort * 4;
  l.wbox = l.rankof + nsort * 4;
  l.unused = l.wbox + 2 * (unsigned)K * 16;
  l.qzt = l.unused + 8 * (unsigned)K;
  l.qzw = l.qzt + NQ * 4;
  l.wR = l.qzw + NQ * 4;
  l.plk = l.wR + (unsigned)K * 4;
  l.plm = l.plk + (form == K3pStream::TwoPass ? (unsigned)K * 4 : 0u);
  l.end = l.plm + (form == K3pStream::TwoPass ? (unsigned)K * 4 : 0u);
  return l;
}

// ---- overlays on that carve
// the bitonic sort's two exchange buffers (one word per thread each), in frag before the scatter
__host__ __device__ constexpr size_t k3p_bitonic_bytes() { return (size_t)2 * IA_WGH * sizeof(unsigned); }
static_assert(k3p_bitonic_bytes() <= k3p_lds(1, false, K3pStream::TwoPass, 512, 1).qlo, "the smallest fragment area holds them");
// the subset merge's area, from frag on (it may run past the carve: the launch then sizes for it):
// [NW][QT][32] Top2, or with two passes every lane's (b1, T, row): [NW][QT][64] x 3 words
__host__ __device__ constexpr size_t k3p_red_top2_bytes(int QT) { return (size_t)K3H_NW * QT * IA_TILE * sizeof(Top2); }
__host__ __device__ constexpr size_t k3p_red_lanes_bytes(int QT) { return (size_t)K3H_NW * QT * IA_WAVE * 12; }
__host__ __device__ constexpr size_t k3p_red_bytes(int QT, K3pStream form) {
  return form == K3pStream::TwoPass && k3p_red_lanes_bytes(QT) > k3p_red_top2_bytes(QT) ? k3p_red_lanes_bytes(QT)
                                                                                        : k3p_red_top2_bytes(QT);
}
// the launch's dynamic LDS
__host__ __device__ constexpr size_t k3p_dyn_bytes(int QT, bool pre, K3pStream form, int Mpad, int K) {
  return k3p_lds(QT, pre, form, Mpad, K).end > k3p_red_bytes(QT, form) ? k3p_lds(QT, pre, form, Mpad, K).end
                                                                       : k3p_red_bytes(QT, form);
}
// two passes: the waves' LDS-DMA rings ([NW][3] slots, a static array of the kernel) and what the
// second pass stages in them: the query lo pieces [QT][KS][64], then the row map [K][32]
__host__ __device__ constexpr size_t k3p_ring_h16x8() { return (size_t)K3H_NW * 3 * IA_HSLOT; }
__host__ __device__ constexpr size_t k3p_ring_bytes() { return k3p_ring_h16x8() * sizeof(h16x8); }
__host__ __device__ constexpr size_t k3p_stage_lo_h16x8(int QT) { return (size_t)QT * IA_K3P_KS * IA_WAVE; }
__host__ __device__ constexpr size_t k3p_stage_bytes(int QT, int K) {
  return k3p_stage_lo_h16x8(QT) * sizeof(h16x8) + (size_t)K * IA_TILE * sizeof(int);
}
// whether a launch can take the two-pass form: the staging fits the rings, and the kernel's
// static LDS (the rings and its counters) with this launch's dynamic part fits the CU's 160 KiB
constexpr size_t IA_LDS_CU = 160 * 1024;
// the kernel's static LDS, rounded to 16 bytes: the ring (one pass: a 1-element placeholder), four
// [NW] per-wave tallies and three counters (k3h_prune3 asserts that its statics are within this)
__host__ __device__ constexpr size_t k3p_static_bytes(K3pStream form) {
  return ((form == K3pStream::TwoPass ? k3p_ring_bytes() : sizeof(h16x8)) + 4 * K3H_NW * sizeof(unsigned) + 3 * sizeof(int) + 15) & ~(size_t)15;
}
__host__ __device__ constexpr bool k3p_two_pass_fits(int QT, bool pre, int Mpad, int K, size_t static_lds) {
  return k3p_stage_bytes(QT, K) <= k3p_ring_bytes() && static_lds + k3p_dyn_bytes(QT, pre, K3pStream::TwoPass, Mpad, K) <= IA_LDS_CU;
}

// ---- pins of the format at QT 11, K 128 (in-kernel sort: a step of 352 queries): a change that
// moves one of them changes what the launches allocate and which of them take the two-pass form
static_assert(k3p_lds(11, false, K3pStream::TwoPass, 352, 128).end == 71824, "in-kernel sort, two passes");
static_assert(k3p_red_bytes(11, K3pStream::TwoPass) == 67584, "its reduction area");
static_assert(k3p_lds(11, true, K3pStream::TwoPass, 4096, 128).end == 69008, "presorted, two passes");
static_assert(k3p_lds(11, false, K3pStream::Whole, 352, 128).end == 115856, "in-kernel sort, whole tiles");
static_assert(k3p_lds(11, false, K3pStream::HiOnly, 352, 128).end == 115856, "in-kernel sort, hi-only stream");
static_assert(k3p_lds(11, true, K3pStream::Whole, 4096, 128).end == 113040, "presorted, whole tiles");
// the largest launch the host admits (presorted whole tiles, QT 11, K = IA_K3P_MAXK_LDS) fits a
// CU's LDS next to the kernel's static part
static_assert(k3p_dyn_bytes(11, true, K3pStream::Whole, 4096, IA_K3P_MAXK_LDS) == 152464, "the worst case");
static_assert(k3p_dyn_bytes(11, true, K3pStream::Whole, 4096, IA_K3P_MAXK_LDS) + k3p_static_bytes(K3pStream::Whole) <= IA_LDS_CU, "and it fits");
static_assert(k3p_static_bytes(K3pStream::TwoPass) == 86160, "the two-pass forms' static LDS");
