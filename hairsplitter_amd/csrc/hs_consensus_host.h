// hs_consensus_host.h -- the consensus of a polishing bundle (include/hairsplitter_hip.h: hs_polish_consensus): a vote per backbone column and
// per insertion slot over the pieces hs_polish_inputs cut, stated once for the host and the device. The reference shells out to minimap2 and
// racon here (tools.cpp:317-...): it has no counterpart to compare against, the rule is ours. DESIGN 4.9g.
// No device code and no HIP call in here or in hs_consensus_host.cpp: tests/harness/consensus_selftest.cpp builds both into a program of its own.
//
// The defaults of hs_consensus_params (min_cov 3, max_ins 32) are PLACEHOLDERS. They are not tuned.
//
//   bundle           backbone text B[0..L); pieces k with text P_k, s_k = piece_sam_pos (1-based on B), CIGAR words len << 4 | op.
//   walk             t = s_k - 1, q = 0. M: column t gets a vote for P_k[q], both advance. D: column t gets a vote for deletion, t advances.
//                    I: q advances. Every other op moves nothing and votes nothing. Votes at t >= L are dropped and the walk ends there.
//                    A piece covers column t if it voted there (M or D).
//   skipped pieces   empty; flagged HS_POLISH_START_BEYOND_SEQ; sum(M + I) != its base count; s_k - 1 >= L. Counted (n_skipped).
//   column t         cov = pieces that cover t. cov < min_cov: the column keeps the byte B[t] (n_low). Otherwise the largest count among
//                    A C G T deletion wins; on equal counts B[t]'s code if it is among the tied, else the first of A C G T deletion.
//                    A winning deletion emits nothing (n_del); a winning base other than B[t]'s code is a substitution (n_sub).
//   slot t           between the columns t - 1 and t, 1 <= t <= L - 1. span = pieces that cover both; an I op votes there only if its piece
//                    covers both, consecutive I ops between the same two column events being one insertion (its bases are one stretch of
//                    P_k: nothing but I consumes read bases between two column events). nins = pieces with an insertion there.
//                    The slot wins iff span >= min_cov and 2 nins > span. An insertion longer than max_ins votes with its first max_ins
//                    bases and the length max_ins. Emitted length l = the most frequent length among the voters, the smaller on a tie;
//                    base j < l = the most frequent code at offset j over the voters of length > j, A < C < G < T on a tie (n_ins_bases += l).
//   text             per column: the slot's insertion, then the column's base. Column t BEGINS in front of its slot's insertion:
//                    trim_start / trim_end = the offsets at which the columns min(overhang_left, L) and L - min(overhang_right, L) begin
//                    (column L: the end of the text).
//   bytes            A C G are the codes 0 1 2, every other byte is T (sequence.cpp:13-23).
#ifndef HS_CONSENSUS_HOST_H
#define HS_CONSENSUS_HOST_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/hairsplitter_hip.h"

#include "hs_rules.h"      // HS_HD

namespace hs {

enum { CONS_DEL = 4, CONS_KEEP = 5 };                                  // what a column emits besides the codes 0..3: nothing, the byte B[t]
enum { CONS_COL_CODE = 7, CONS_COL_SLOT = 8, CONS_COL_SUB = 16 };      // a decided column's byte: what it emits, "its slot wins", "a substitution"
enum { CONS_ROW_VOTE = 7, CONS_ROW_INS = 8, CONS_ROW_PREV = 16 };      // a row byte: the vote, "an insertion of the piece in the slot before", "the piece covers t - 1 too"

HS_HD inline bool consensus_params_valid(const hs_consensus_params& p) { return p.min_cov >= 1 && p.max_ins >= 1 && p.max_ins <= 64; }
HS_HD inline int cons_code(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3; }
HS_HD inline uint8_t cons_letter(int code) { return (uint8_t)("ACGT"[code & 3]); }
// how far an op moves the column cursor and the read cursor
HS_HD inline int64_t cons_col_advance(uint32_t op) { const uint32_t c = op & 15u; return c == 0 || c == 2 ? (int64_t)(op >> 4) : 0; }
HS_HD inline int64_t cons_read_advance(uint32_t op) { const uint32_t c = op & 15u; return c == 0 || c == 1 ? (int64_t)(op >> 4) : 0; }

// what the walk of one piece comes to, without the votes: is it skipped, how many columns it covers (clipped at L) and how many insertions
// vote (a slot each). The device's rows and records are laid out by these. long_cigar: the M I D lengths sum beyond 2^31 - 1 (the caller refuses).
struct ConsPiecePlan { bool skipped, long_cigar; int32_t n_cols, n_ins; };
HS_HD inline ConsPiecePlan cons_piece_plan(const uint32_t* cigar, int64_t n_ops, int64_t n_bases, int32_t flags, int64_t s, int64_t L) {
    ConsPiecePlan p = {true, false, 0, 0};
    int64_t rd = 0, all = 0;
    for (int64_t i = 0; i < n_ops; ++i) { rd += cons_read_advance(cigar[i]); all += cons_read_advance(cigar[i]) + cons_col_advance(cigar[i]); }
    if (all > 0x7fffffff) { p.long_cigar = true; return p; }
    if (n_bases == 0 || (flags & HS_POLISH_START_BEYOND_SEQ) || rd != n_bases || s - 1 >= L) return p;
    p.skipped = false;
    const int64_t room = L - (s - 1);
    int64_t cols = 0, pending = 0;
    for (int64_t i = 0; i < n_ops && cols < room; ++i) {
        const uint32_t c = cigar[i] & 15u;
        const int64_t len = (int64_t)(cigar[i] >> 4);
        if (len == 0) continue;
        if (c == 1) pending += len;
        else if (c == 0 || c == 2) {
            if (pending > 0 && cols > 0) ++p.n_ins;
            pending = 0;
            cols += len;
        }
    }
    p.n_cols = (int32_t)(cols < room ? cols : room);
    return p;
}

// the column rule: v[0..3] the bases' votes, v[4] the deletions'; ref = cons_code(B[t]). Returns 0..3, CONS_DEL or CONS_KEEP
HS_HD inline int cons_column_decide(const uint32_t v[5], int ref, int32_t min_cov) {
    const uint64_t cov = (uint64_t)v[0] + v[1] + v[2] + v[3] + v[4];
    if (cov < (uint64_t)min_cov) return CONS_KEEP;
    int best = 0;
    uint32_t top = v[0];
    for (int c = 1; c < 5; ++c) if (v[c] > top) { top = v[c]; best = c; }
    const uint32_t of_ref = ref == 0 ? v[0] : ref == 1 ? v[1] : ref == 2 ? v[2] : v[3];      // (no indexed read: the device keeps v in registers)
    return of_ref == top ? ref : best;
}
// the decided column's byte (without its slot)
HS_HD inline uint8_t cons_column_byte(const uint32_t v[5], uint8_t b, int32_t min_cov) {
    const int ref = cons_code(b), w = cons_column_decide(v, ref, min_cov);
    return (uint8_t)(w | (w < 4 && w != ref ? CONS_COL_SUB : 0));
}
HS_HD inline bool cons_slot_wins(uint32_t nins, uint32_t span, int32_t min_cov) { return span >= (uint32_t)min_cov && 2 * (uint64_t)nins > span; }
HS_HD inline int32_t cons_ins_cap(int64_t len, int32_t max_ins) { return len > max_ins ? max_ins : (int32_t)len; }

// a winning slot's table: [0 .. max_ins] voters per (capped) length, then 4 counts per offset
HS_HD inline int32_t cons_table_words(int32_t max_ins) { return max_ins + 1 + 4 * max_ins; }
HS_HD inline int32_t cons_ins_length(const uint32_t* tab, int32_t max_ins) {
    int32_t best = 0;
    for (int32_t l = 1; l <= max_ins; ++l) if (tab[l] > tab[best]) best = l;      // (tab[0] is 0: no voter has length 0)
    return best;
}
HS_HD inline int cons_ins_base(const uint32_t* tab, int32_t max_ins, int32_t j) {
    const uint32_t* c = tab + max_ins + 1 + 4 * j;
    int best = 0;
    for (int k = 1; k < 4; ++k) if (c[k] > c[best]) best = k;
    return best;
}

// one call on the host (hs_consensus_host.cpp): the arrays of hs_polish_consensus_arrays, the bundles strided over n_threads
struct ConsensusHost {
    std::vector<int64_t> cons_off;
    std::vector<uint8_t> cons;
    std::vector<int32_t> trim_start, trim_end, n_sub, n_del, n_ins_bases, n_low, n_skipped;
    int64_t n_ins_records = 0, n_ins_slots = 0;
};
// the checks both halves make before any work: HS_OK or HS_EINVAL with a message
int consensus_check(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                    const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                    const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, std::string& err);
int consensus_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                   const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                   const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, int n_threads, ConsensusHost& out, std::string& err);
// the same call, handing out two figures per column t of every bundle, t in [0, L] (cols may be null; hs_refine_host.h reads them): col_begin[t], where
// column t begins in the bundle's text (column L: its end), and col_ins[t], the inserted bases in front of column t. col_off[b]: where bundle b's L + 1 entries lie.
struct ConsensusColumns { std::vector<int64_t> col_off; std::vector<int32_t> col_begin, col_ins; };
int consensus_host_columns(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left, const int32_t* overhang_right,
                           const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases,
                           const int64_t* cig_off, const uint32_t* cigar, const hs_consensus_params& prm, int n_threads, ConsensusHost& out, ConsensusColumns* cols,
                           std::string& err);
// a ConsensusHost as the malloc'd result of the C ABI (nullptr: out of memory)
hs_consensus_result* consensus_result_from_host(const ConsensusHost& h);

}  // namespace hs

#endif
