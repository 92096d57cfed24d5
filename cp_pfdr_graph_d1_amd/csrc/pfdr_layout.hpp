// The contribution layouts of the quadratic session's vertex and edge sweeps:
// their formats (stated here and nowhere else), the two structs that own
// the device tables, and (pfdr_layout.hip) the kernels and host code that
// build them.  The per-iteration readers are tile_sum*, split_sum and
// k_edge_sweep_tl in pfdr_quadratic_kernels.hpp.
#pragma once
#include "pfdr_graph.hpp"

namespace pfdr {

struct Halo;

// ---------------------------------------------- tiled DR contributions --
// Large single-GPU graphs store their edges in TILE order: sorted by
// (u block, v block, edge), 256-vertex blocks (the vertex sweep's).  The
// edge sweep then writes both contributions W*Z at the edge's position
// (wz[p] u end, wz[E + p] v end) as plain streams, and every vertex block
// finds ALL of its contributions in a few contiguous runs: the u ends of
// its own block's edges (wz[ustart[b] .. ustart[b+1]), one run) and the
// v ends of the (u block, b) tiles (runs of wz[E + p] listed in tptr /
// tstart / tlen).  Each run is read once, coalesced, by exactly one
// workgroup; every entry carries its slot in the block's CSR-ordered list
// (d2, 16 bits, the CSR position of (edge, side) minus the block's first),
// so staging puts each contribution where the reference's (e, side) order
// wants it, and each lane then adds its vertex's slots in order -- the sums
// of gather_sum / split_sum bit for bit, without a single gathered load.
constexpr int kTileCap = 4096;  // staged entries per vertex block (LDS: GatherCap)

// Each vertex's slots [my0, my0 + deg) in the block's list come from its
// degree (deg8: one byte per vertex, < 256 in every tiled block -- tok)
// by a block scan, instead of two CSR pointers (1 B per vertex, not 4).
// The slots are 12-bit (a tiled block lists at most kTileCap = 4096
// contributions), packed eight to a 12-byte group (Slots12), and the runs
// are staged a group at a time: one 12-byte slot load beside the group's
// contributions (two 16-byte loads f32, four f64), from the aligned group
// at or below each run's start, elements outside the run dropped.  The
// contribution arrays carry one spare group at their end for the last
// run's tail.
constexpr int kTileRuns = 128;  // v-end runs per vertex block
constexpr int kSlotGroup = 8;   // contributions per packed slot group
struct alignas(4) Slots12 { unsigned w[3]; };  // 8 x 12 bits, little-endian
__device__ __forceinline__ int slot12(const Slots12 &g, int i) {
    const unsigned long long lo = g.w[0] | ((unsigned long long)g.w[1] << 32);  // bits 0..63
    const unsigned long long hi = g.w[1] | ((unsigned long long)g.w[2] << 32);  // bits 32..95
    return i < 5 ? (int)((lo >> (12 * i)) & 0xfff) : (int)((hi >> (12 * i - 32)) & 0xfff);
}
// the first n (<= kSlotGroup) of the slots s[0..8) packed into one group:
// slot i at bits [12 i, 12 i + 12), the others 0
__host__ __device__ inline Slots12 pack_slots12(const unsigned short *s, long n) {
    Slots12 g{};
    for (int q = 0; q < kSlotGroup && q < n; q++) {
        const unsigned x = s[q] & 0xfffu;
        const int w = 12 * q / 32, bit = 12 * q % 32;
        g.w[w] |= x << bit;
        if (bit > 20) g.w[w + 1] |= x >> (32 - bit);  // (across two words)
    }
    return g;
}

// A tiled block (tok 1) with at most kRecRuns v-end runs is a RECORD block
// (tok 2): [u start, u count, runs, (start, length) x runs] in kTileRec
// ints of trec, so the block's metadata is ONE load round (the run table
// otherwise costs two dependent ones, tptr then tstart / tlen, and a
// barrier).  Blocks whose lists do not fit (tok 0) gather through the CSR.
constexpr int kRecRuns = 14, kTileRec = 32;
constexpr int kPrec = 16;  // runs per block in prec: the u run, then up to 15 v runs

// ------------------------------------------------ slot patterns -------
// On regular graphs most record blocks' runs carry the same slot sequences
// (on C2 every interior block is one x-row of the grid; on C5 the 640-vertex
// rows give five phases).  A run's PATTERN = (its first address mod 8, its
// length, its slots); the distinct patterns go to a small table of packed
// groups (ptab, aligned as each run's groups are) and each record block gets
// the table offset of every run (prec: 16 ints beside its record), so the
// vertex sweep reads no per-entry slot stream (12 B per 8 contributions).
// Runs that hash alike share a pattern only when their lengths and first
// addresses mod 8 agree and their slots are equal entry by entry; the table
// is off when the patterns do not repeat (the jittered headline) or
// PFDR_TILE_PATTERNS=0.
// run q of a record r (0: the u run): its first address in wz and its length
__host__ __device__ inline bool rec_run(const int *r, long E, int q, long &A, int &len) {
    if (q > r[2]) return false;
    A = q ? E + r[1 + 2 * q] : r[0];
    len = q ? r[2 + 2 * q] : r[1];
    return true;
}

// --------------------------------------------- edge-block records -----
// The record of every edge block of k_edge_sweep_tl (EB edges), kErec ints:
// rec[0..3]: ub0 (first u block), nub, nruns (0: more than kEbRuns, the
// block reads Ev), uoff (smallest u end - ub0 * 256); the staged u range is
// [ub0 * 256 + uoff, + span), span = largest - smallest + 1; then where each
// further u block starts and the runs of equal v block in edge order, starts
// relative to the block's first edge, padded past the last run.  Every edge
// names both ends by one byte each (luv: u mod 256 | v mod 256 << 8).
//
// A partitioned rank's edge block that straddles its interior / boundary cut
// (the edges with a ghost end are sorted after the interior ones, each part
// by u block) sees the u block DROP inside the block.  Its u ends are not a
// few consecutive blocks from ub0 on, so the block is marked unstaged (nub =
// kErecNoStage: k_edge_sweep_tl reads Eu) and no u-block start is recorded
// -- u blocks below ub0 would otherwise index before the record.
constexpr int kEbRuns = 20;  // v-block runs in an edge block's record
constexpr int kErecU = 4;    // rec[4]: staged span; rec[4 + q]: start of u block ub0 + q
                             // (q = 1..3; INT_MAX if q >= nub)
constexpr int kErecS = 8;    // rec[kErecS + 2r]: start of run r (INT_MAX if r >= nruns), + 1: its v base
constexpr int kErec = kErecS + 2 * kEbRuns;
constexpr int kErecNoStage = 1 << 30;  // nub of a block whose u blocks are not nondecreasing

// The tables of a tile-ordered session, built around the incidence CSR:
// order() before it, build() after it.
struct TileLayout {
    DevBuf<Slots12> slots;        // the slot of every contribution address, packed
    DevBuf<unsigned char> deg8;   // CSR entries per vertex
    DevBuf<unsigned short> luv;   // both ends mod 256 (k_edge_sweep_tl)
    DevBuf<int> erec;             // per edge block: u blocks and v runs (k_edge_sweep_tl)
    DevBuf<int> ustart, tptr, tstart, tlen;  // the runs each block stages
    DevBuf<int> tok, trec;        // per block: 0 gathered / 1 tiled / 2 record; its record
    DevBuf<Slots12> ptab;         // slot patterns of the record blocks' runs
    DevBuf<int> prec;             // per record block: its runs' offsets into ptab
    long Eint = 0;      // edges [0, Eint) have no ghost end (a partitioned rank; else E)
    int vpair_cap = 0;  // pair vertex sweep: entries of the largest record block (0: off)
    long tiled_blocks = 0, record_blocks = 0, slot_patterns = 0;

    // Eu / Ev into tile order, stable in the current one.  ids (null:
    // e_offset + position) = the edges' ids for the incidence keys, the
    // original ones of a relabelled graph or a partitioned rank's global
    // ones; eo = those of the new order; emap = each edge's position in the
    // caller's per-edge arrays.  A partitioned rank puts the edges with a
    // ghost end after the others (the interior ones overlap the halo pull),
    // counts Eint and renumbers the halo's push addresses.
    void order(long E, int V, int Vg, DevBuf<int> &Eu, DevBuf<int> &Ev, const unsigned *ids,
               long e_offset, DevBuf<unsigned> &eo, DevBuf<int> &emap, Halo *halo, hipStream_t s);
    // slots, runs, records, deg8, luv, erec, the pair capacity (PFDR_VPAIR)
    // and the patterns (PFDR_TILE_PATTERNS) of elements of elem bytes
    void build(long E, int V, const int *Eu, const int *Ev, const Incidence &inc, const Halo *halo,
               size_t elem, hipStream_t s);
    // what the session reports in device_bytes: ptab and prec are NOT
    // counted (an omission kept so the reported number does not move)
    size_t bytes() const {
        return slots.n * sizeof(Slots12) + luv.n * 2 + deg8.n +
               (ustart.n + tptr.n + tstart.n + tlen.n + tok.n + trec.n + erec.n) * 4;
    }

  private:
    void build_patterns(long E, int V, const unsigned short *d2, long n, hipStream_t s);
};

// Split incidence (split_sum) of a graph whose edges are sorted by their u
// end: u-run offsets, per-vertex order masks, addresses of the other entries,
// per-block path flag.  Blocks that do not qualify keep the CSR gather.
struct SplitLayout {
    DevBuf<int> uptr, blkok;
    DevBuf<unsigned> mask, oidx;
    long split_blocks = 0;
    // cap: entries of each of a block's two staged lists (half the LDS list)
    void build(long E, int V, const int *Eu, const Incidence &inc, int cap, hipStream_t s);
    size_t bytes() const { return (uptr.n + mask.n + oidx.n + blkok.n) * 4; }
};

}  // namespace pfdr
