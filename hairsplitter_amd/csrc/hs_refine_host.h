// hs_refine_host.h -- polishing passes (include/hairsplitter_hip.h: hs_polish_haplotypes_refined): a pass p >= 2 realigns every piece of a bundle to
// the consensus pass p - 1 made of it and votes again with that consensus as the backbone. Stated once for the host and the device. The reference
// runs minimap2 a second time in front of racon here (tools.cpp:317-...); the rule is ours. DESIGN 4.9i.
// No device code and no HIP call in here or in hs_refine_host.cpp: tests/harness/refine_selftest.cpp builds both into a program of its own.
//
//   from pass p - 1   K, the bundle's untrimmed consensus; per column t in [0, L]: col_begin[t], where column t begins in K (in front of its slot's
//                     insertion; col_begin[L] = |K|), and col_ins[t], the inserted bases in front of column t (0 for t = 0 and a slot that did not win).
//   window            a piece pass p - 1 did not skip whose plan has n_cols >= 1 (hs::cons_piece_plan, first column s0):
//                     ws = col_begin[s0] + col_ins[s0], we = col_begin[s0 + n_cols]. The piece did not span the slot in front of its first column:
//                     that insertion is not in its window. Every other piece has no window (-1, -1).
//   alignment         query = the piece through hs::cons_code, target = K[ws, we) through the same; edlibAlign(query, target, k = -1, NW, PATH); the
//                     words are hs_moves_to_cigar's without clips (moves 0 and 3: M, 1: I, 2: D). we == ws: the one word n_bases << 4 | I and no
//                     aligner call. A pair the aligner has no path for gets no words; a piece without a window gets none. The plan of pass p skips
//                     both by its own rule (sum(M + I) != its base count).
//   inputs of pass p  backbone K; overhang_left = trim_start, overhang_right = |K| - trim_end; piece_sam_pos = ws + 1 (1 without a window); flags,
//                     bases, min_cov and max_ins unchanged; CIGAR = the words above. The pass is hs_consensus_host.h's rule as it stands.
#ifndef HS_REFINE_HOST_H
#define HS_REFINE_HOST_H

#include "hs_consensus_host.h"

namespace hs {

// has the piece a window? (what pass p - 1's plan says of it)
HS_HD inline bool refine_has_window(bool skipped, int32_t n_cols) { return !skipped && n_cols >= 1; }
// the window from the three column figures it reads: col_begin[s0], col_ins[s0], col_begin[s0 + n_cols]
HS_HD inline void refine_window(int64_t begin_first, int64_t ins_first, int64_t begin_behind, int64_t* ws, int64_t* we) { *ws = begin_first + ins_first; *we = begin_behind; }
// the word of a piece whose window is empty (a length beyond the word's 28 bits does not sum to the base count: the plan skips the piece)
HS_HD inline uint32_t refine_empty_word(int64_t n_bases) { return ((uint32_t)n_bases << 4) | 1u; }
// a move of the aligner as a CIGAR op (hs_moves_to_cigar)
HS_HD inline uint32_t refine_move_op(uint8_t move) { return move == 1 ? 1u : move == 2 ? 2u : 0u; }
// the next pass's fields of a piece and of a bundle
HS_HD inline int32_t refine_sam_pos(int64_t ws) { return ws < 0 ? 1 : (int32_t)(ws + 1); }
HS_HD inline int32_t refine_overhang_left(int32_t trim_start) { return trim_start; }
HS_HD inline int32_t refine_overhang_right(int64_t cons_len, int32_t trim_end) { return (int32_t)(cons_len - trim_end); }

// one pass on the host and what the next one needs of it: the consensus, the two column arrays, every piece's window (counted from its bundle's text)
struct RefinePlanHost {
    ConsensusHost cons;
    ConsensusColumns cols;
    std::vector<int64_t> win_start, win_end;      // [n_pieces]; -1 / -1: no window
};
int refine_plan_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                     const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                     const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, int n_threads, RefinePlanHost& out, std::string& err);
// a RefinePlanHost as the malloc'd result of the C ABI (nullptr: out of memory)
hs_refine_plan* refine_plan_from_host(const RefinePlanHost& h);

}  // namespace hs

#endif
