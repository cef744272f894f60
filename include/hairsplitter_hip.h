/*
 * hairsplitter_hip.h -- C ABI of the MI355X (gfx950) implementation of HairSplitter's hot path
 * (HS_call_variants -> HS_separate_reads). Plain pointers and sizes only; no C++/torch types.
 *
 * The reference has no FFI: its boundary is two executables and five text formats.
 * The drop-in executables shipped here (hairsplitter_amd/bin/HS_call_variants, HS_separate_reads) are thin
 * hosts over this library; every entry point below names the reference function (file:line under
 * /root/reference/src) whose work it replaces, so a maintainer could also call it in-process.
 *
 * Conventions
 *  - Pointers named d_* are DEVICE (HBM) pointers, h_* are host pointers. `stream` is a hipStream_t passed
 *    as void* (NULL = the default stream). Kernel-level calls are asynchronous on `stream`.
 *  - Every function returns 0 on success, a negative HS_E* code otherwise; hs_last_error() gives the text.
 *  - Sequences are 1 byte per base, codes A=0 C=1 G=2 T=3 (non-ACG input bases become T exactly like the
 *    reference's 2-bit Sequence, sequence.cpp:13-23). Reads are stored as sequenced (FASTA orientation); the
 *    kernels reverse-complement on the fly for records whose strand is 0 (call_variants.cpp:108-115).
 *  - CIGARs are BAM-style uint32 (len << 4 | op), op: M=0 I=1 D=2 N=3 S=4 H=5 P=6 '='=7 X=8.
 *  - "record" = one kept SAM line = one read index n of a contig (call_variants.cpp:85-86). Records are
 *    grouped by contig, in SAM file order inside a contig.
 */
#ifndef HAIRSPLITTER_HIP_H
#define HAIRSPLITTER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HS_OK 0
#define HS_ENODEVICE (-1)   /* no HIP device / extension unusable: the product never falls back to a CPU path */
#define HS_EINVAL (-2)
#define HS_EHIP (-3)
#define HS_EIO (-4)
#define HS_EFORMAT (-5)

/* ------------------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------------------- */
const char* hs_version(void);
const char* hs_last_error(void);
int hs_device_count(void);                       /* hipGetDeviceCount; 0 when there is no GPU */
int hs_warmup(void);                             /* runtime + context + code-object load (first launch); returns the device count.
                                                    The executables run it on a side thread while they parse their inputs. */
int hs_set_device(int device);
int hs_device_synchronize(void);
/* raw HBM helpers so that hosts without a HIP binding (ctypes, cgo, JNI) can stage buffers */
int hs_malloc(void** d_ptr, size_t bytes);
int hs_free(void* d_ptr);
int hs_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int hs_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int hs_memset(void* d_ptr, int value, size_t bytes);
/* event timing on the stream the kernels run on (bench.py's roofline leg) */
int hs_event_create(void** ev);
int hs_event_destroy(void* ev);
int hs_event_record(void* ev, void* stream);
int hs_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronises on ev_stop */

/* ------------------------------------------------------------------------------------------------
 * Per-kernel accounting of everything the stage drivers launch (bench.py's roofline leg): every launch is bracketed by HIP
 * events on the stream it runs on; the elapsed times, the number of launches and the ALGORITHMIC bytes of each launch
 *  are accumulated per kernel family, process-wide, until hs_kernel_stats_reset().
 * ---------------------------------------------------------------------------------------------- */
#define HS_NKERNELS 28
enum {   /* one slot per kernel of the path (a slot's helper launches -- prefix scans, block sums -- are counted with it) */
    HS_K_CIGAR_SCAN = 0, HS_K_PILEUP, HS_K_COLUMN_STATS, HS_K_COLUMNS_COMPACT, HS_K_GATHER_COLUMNS, HS_K_COLUMN_TOP3, HS_K_CANDIDATES_SCAN,
    HS_K_PACK_COLUMNS, HS_K_PARTITION_TRANSPOSE, HS_K_PARTITION_LANES, HS_K_PARTITION_TEST, HS_K_SNP_SELECT, HS_K_WINDOW_MASKS,
    HS_K_SNP_PLANES, HS_K_SIMDIFF, HS_K_GRAPH_ROWS, HS_K_GRAPH_CSR, HS_K_VISIT_LISTS, HS_K_CW_SEED_SETS, HS_K_CW_SEEDED, HS_K_CW_SEEDED_WIDE,
    HS_K_WINDOW_TAIL, HS_K_CW_LOCAL, HS_K_ROBUST_PARTITIONS, HS_K_OTHER, HS_K_CAND_BITS, HS_K_SHIP, HS_K_PARTITION_GROUPED
};
typedef struct hs_kernel_stats {
    double ms[HS_NKERNELS];        /* sum of the launch durations (hipEventElapsedTime) */
    int64_t launches[HS_NKERNELS];
    int64_t bytes[HS_NKERNELS];    /* sum of the algorithmic bytes of the launches */
} hs_kernel_stats;
const char* hs_kernel_name(int k);          /* name of the (dominant) kernel of family k as rocprofv3 prints it */
void hs_kernel_stats_reset(void);
void hs_kernel_stats_get(hs_kernel_stats* out);
/* Host waits for the device since the library was loaded: each is one round trip in the chain of a contig group (bench.py reports
 * them per step). The time spent in them is only accumulated under HS_TIMING. A wait polls hipStreamQuery and sleeps 25 us between two
 * looks; for the duration of the wait the calling thread's timer slack is set to 1 us (prctl PR_SET_TIMERSLACK; HS_TIMER_SLACK_NS=0: not
 * touched) and the thread's own value is put back before the call returns. */
/* Timing events of the library (two per kernel launch for hs_kernel_stats, a few per phase for the t_kernel_* fields) are recorded on every
 * pipeline step by default; hs_kernel_stats_every(n) records them on every n-th step only (steps counted from this call; hs_pipeline_select /
 * hs_pipeline_run_fused begin a step). hs_kernel_stats then holds the launches of the timed steps; the t_kernel_* fields of an untimed step are 0.
 * About 1200 event records per step of the 500-contig job cost it 1.3 ms of 16.9. */
void hs_kernel_stats_every(int32_t n);
void hs_host_wait_stats(int64_t* n_waits, double* ms_in_waits);

/* ------------------------------------------------------------------------------------------------
 * K1 -- pileup.  Replaces generate_msa (call_variants.cpp:50-437) + convert_cigar (tools.cpp:27-57).
 * One wavefront per task (a range of alignment events of one record). Launches K0 (CIGAR scan: fills d_chunk_scratch with the
 * cursors at every 64-op chunk and flags the records that hold a clip between aligned bases), the packed pileup kernel (four
 * events per lane) over the task list and the per-event kernel over the flagged records. For record r with reference start pos[r]:
 *   d_pile[pile_off[r] + (q - pos[r])] = 33 + 5*i(c-2) + i(c-1) + 25*i(c0)   for every M/=/X/D event at q < L
 * (i() = index in "ACGT-", previous chars initialised C,G as call_variants.cpp:212-214 leave them).
 * d_rec_stats[r] = {q_end, n_err, n_len, n_events}: final reference cursor (call_variants.cpp:354) and the number
 * of +1's applied to totalDistance / totalLengthOfAlignment (call_variants.cpp:255-257,305-306,337-338).
 * ---------------------------------------------------------------------------------------------- */
int hs_pileup(const uint8_t* d_contig_seq, const int64_t* d_contig_off,   /* [C+1] */
              const uint8_t* d_read_seq, const int64_t* d_read_off,        /* [NR+1] */
              const int32_t* d_rec_read, const int32_t* d_rec_contig, const int32_t* d_rec_pos,
              const uint8_t* d_rec_strand, const int64_t* d_rec_cig_off,   /* [NREC+1] */
              const uint32_t* d_cigar, const int64_t* d_pile_off,          /* [NREC+1] */
              int32_t n_rec,
              /* launch plan from hs_pileup_plan (work is split in equal ranges of alignment events, not per record) */
              const int64_t* d_rec_chunk_off, int32_t* d_chunk_scratch /* [4 * rec_chunk_off[NREC]] */,
              const int32_t* d_task_rec, const int32_t* d_task_ev0, int32_t n_tasks, int32_t ev_per_task,
              uint8_t* d_pile, int32_t* d_rec_stats /* [NREC*4] */, void* stream);

/* Host-side launch plan of hs_pileup, from host copies of the CIGARs (the per-record aggregates parse_SAM also
 * derives, input_output.cpp:486-505): rec_chunk_off[r] = number of 64-op chunks before record r; tasks = (record,
 * first event) pairs covering every record in ranges of ev_per_task events. The two task arrays are malloc'ed;
 * release them with hs_free_host. */
int hs_pileup_plan(const int64_t* h_rec_cig_off, const uint32_t* h_cigar, int32_t n_rec, int32_t ev_per_task,
                   int64_t* h_rec_chunk_off /* [NREC+1] out */, int32_t* n_tasks, int32_t** h_task_rec, int32_t** h_task_ev0);
void hs_free_host(void* p);

/* ------------------------------------------------------------------------------------------------
 * K2 -- per-position code histogram and top-5.  Replaces the counting half of call_variants
 * (call_variants.cpp:471-507): for every contig position the five most frequent pileup codes.
 * Output record (16 B / position): u8 key[4]; u16 cnt[5]; u16 depth -- ordered by (count desc, code asc);
 * missing entries have key 0 / count 0. The reference's tie order (robin_hood iteration order + std::sort) is
 * applied afterwards by the host only where it is observable (hs_colstat flags).
 * d_contig_rec_off[C+1] gives each contig's record range; d_rec_qend[r] = exclusive end of record r's pileup.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_colstat {
    uint8_t key[4];
    uint16_t cnt[5];
    uint16_t depth;
} hs_colstat;

/* ------------------------------------------------------------------------------------------------
 * Tile plan for K2 / K3: which records overlap each tile of 256 consecutive positions of the concatenated contigs, in
 * ascending record order. Built on the host from the same per-record aggregates as the pileup layout (one pass over the
 * records; the batch keeps it for its lifetime). entry.first = lane of the tile that holds the record's first position
 * (negative when the record starts in an earlier tile), entry.len = positions the record covers from there,
 * entry.base = offset in the pileup of the byte that lane 0 of the tile would read.
 * Outputs are malloc'ed; release them with hs_free_host.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_tile_entry { int32_t first, len; int64_t base; } hs_tile_entry;
int hs_tile_plan(const int64_t* h_contig_off, int32_t n_contigs, const int32_t* h_contig_rec_off, const int32_t* h_rec_pos,
                 const int32_t* h_rec_qend, const int64_t* h_pile_off, int64_t** tile_off /* [n_tiles+1] */,
                 hs_tile_entry** tile_ent, int32_t** tile_rec, int64_t* n_tiles);
/* K2 on a tile plan in its full-statistics form (total_len = contig_off[C]): d_stats [sum L] or NULL = selection only; optional compact
 * selection (all NULL / 0 to skip): global positions (index into the concatenated contigs) whose second count is >= min_second,
 * unordered, with their depth; *d_sel_count must be 0; max_depth: upper bound on the depth of any position, if known (1..255
 * selects 8-bit LDS counters), 0 = unknown. (The stage drivers run the selection-only form k_column_stats_tiled_dw: see
 * hs_cv_column_pass_taps.) */
int hs_column_stats_tiled(const uint8_t* d_pile, const int64_t* d_tile_off, const hs_tile_entry* d_tile_ent, int64_t total_len,
                          hs_colstat* d_stats, int32_t min_second, int32_t* d_sel_count, int64_t* d_sel_gpos,
                          int32_t* d_sel_depth, int32_t sel_cap, int32_t max_depth, void* stream);
/* Exclusive prefix sum of n non-negative ints into n + 1 64-bit offsets (d_out[n] = total): the CSR offsets of the read
 * graphs (K6) and of the selection list (K2) are built with it. Synchronous with respect to `stream`. */
int hs_exclusive_scan_i32(const int32_t* d_in, int32_t n, int64_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K4 -- SNP column x partition correlation.  Replaces distance(Partition&, Column&) + computeChiSquare
 * (call_variants.cpp:778-967, :1135-1163) as used by loops C and D of keep_only_robust_variants (:721-764).
 * Columns are a CSR as the column pass of stage 3 leaves it (hs_cv_taps); col_k0 / col_k1 their two most frequent codes in the reference's
 * tie order; col_c1 the second count; col_is_cand marks candidate SNPs (loop C). Partitions are dense int8 state
 * arrays over the contig's reads (1, -1, 0, or 2 = read absent); contig c owns partitions [part_off[c], part_off[c+1]).
 * Two kernels: lanes = partitions on a [read][partition] table built on the device (64 partitions per step), then the
 * one-partition-at-a-time form for the few columns whose verdict hinges on the reference's order of tied second alleles.
 * d_keep[i] = 1 if column i is kept by loop C (chi2 > 15 on more than half of its reads) or rescued by loop D
 * (chi2 > 20, both alleles carried by more than four partition reads).
 * ---------------------------------------------------------------------------------------------- */
int hs_column_partition_test(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code,
                             const int32_t* d_col_contig, const uint8_t* d_col_k0, const uint8_t* d_col_k1,
                             const int32_t* d_col_c1, const uint8_t* d_col_is_cand, int32_t n_cols,
                             const int32_t* d_part_off, const int64_t* d_part_state_off, const int8_t* d_part_state,
                             const int32_t* h_contig_n_reads /* HOST, [C]: reads of every contig (length of its state arrays) */, int32_t n_contigs,
                             uint8_t* d_keep, void* stream);
/* Test tap: what the kernels of the LAST hs_column_partition_test call of this thread left to one another -- out[0] columns the first kernel
 * (k_column_partition_lanes) passed on to k_column_partition_grouped, out[1] columns that one passed on whole to k_column_partition_test,
 * out[2] (column, partition) pairs it passed on to k_column_partition_pairs. */
void hs_column_partition_last_counts(int32_t out[3]);

/* ------------------------------------------------------------------------------------------------
 * Test entry: loop A of keep_only_robust_variants (call_variants.cpp:590-638) on prescribed candidate columns, in either form the
 * product has -- form 0: the host's walk (hs::cv_build_cand_bits -> hs::cv_phase_a_host), form 1: the device's (k_loop_a_prepare ->
 * k_loop_a -> k_loop_a_scan -> k_loop_a_pack -> hs::cv_phase_a_import; the plan, the launches and the collection are the ones stage 3
 * queues). All arrays on the HOST. Contig c has the reads [contig_read_off[c], contig_read_off[c + 1]) (read_start / read_end: their
 * alignment's first and exclusive last position) and the columns [contig_col_off[c], contig_col_off[c + 1]) in ascending position:
 * col_pos, the reference code col_k0, and the CSR col_off / col_idx (read indices on the contig, ascending) / col_code.
 * cand_bound: the device walks the contigs with 1 .. cand_bound columns; pool_div: its partition pool holds min(k + 8, k / pool_div + 48)
 * partitions for k columns; light != 0: the columns reach k_loop_a_prepare as a place and a length each in arrays that hold them in
 * another order (the layout of a column pass that keeps no packed entries). None of the three is read from the environment here.
 * Result: on_device[c] (planned for the device), failed[c] (the kernel handed it back); contig c's partitions in creation order are
 * [part_base[c], part_base[c + 1]) -- none for a contig of form 1 that is not on the device or was handed back -- with 9 ints each in
 * rec (left, right, numberOfOccurences, number_of_correlating_snps, lo, hi: first / last read index, reach: largest alignment end,
 * w0, w1: first / last word of ranked reads that holds one) and n_reads entries each in state (2 = absent) / more / less, back to back.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_loop_a_result {
    int32_t n_contigs;
    int32_t* on_device; int32_t* failed;
    int64_t* part_base;
    int32_t* rec;
    int8_t* state; int32_t* more; int32_t* less;
} hs_loop_a_result;
int hs_loop_a_test(int32_t n_contigs, const int32_t* contig_read_off, const int32_t* read_start, const int32_t* read_end, const int64_t* contig_col_off,
                   const int32_t* col_pos, const uint8_t* col_k0, const int64_t* col_off, const int32_t* col_idx, const uint8_t* col_code,
                   int32_t form, int32_t cand_bound, int32_t pool_div, int32_t light, hs_loop_a_result** out, void* stream);
void hs_loop_a_result_destroy(hs_loop_a_result* r);

/* ------------------------------------------------------------------------------------------------
 * V5 -- distance(Partition&, Partition&, threshold_p) of loop B (call_variants.cpp:977-1127) for a list of partition pairs.
 * Partitions as dense arrays one after the other: partition p occupies [part_off[p], part_off[p] + part_n[p]) of d_state
 * (mostFrequentBases in {-1, 0, 1}, 2 = read absent), d_more / d_less (moreFrequence / lessFrequence); the two partitions of a
 * pair belong to the same contig (same part_n). d_sigma3[n], n < 4096 = (float)(0.5 n + 3 sqrt(0.25 n)) as the host forms it.
 * d_out: 8 ints per pair {n00, n01, n10, n11, phased, augmented, valid, comparable}; valid = 0 when a read's vote count is
 * beyond the table (the caller's own walk decides). pair_a = par1, pair_b = par2 of the reference's call.
 * ---------------------------------------------------------------------------------------------- */
int hs_partition_pair_distance(const int8_t* d_state, const int32_t* d_more, const int32_t* d_less, const int64_t* d_part_off, const int32_t* d_part_n,
                               const int32_t* d_pair_a, const int32_t* d_pair_b, int32_t n_pairs, int32_t threshold_p, const float* d_sigma3, int32_t* d_out,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * K5a -- SNP bit-planes for K5 from the SNP columns (separate_reads.cpp:386-405): bit s of row r of d_ref / d_alt = read r
 * carries snp_ref[s] / snp_alt[s]. Columns of all contigs concatenated (CSR); snp_contig[s] = contig of column s,
 * contig_snp_base[c] = first column of contig c; plane_off / words / n_reads as for hs_simdiff (words[c] == 0 skips the contig).
 * Every word of the rows of a contig with words[c] > 0 is written (the planes need no clearing). h_words: the HOST copy of
 * words[] (the launch has one workgroup per contig and four words).
 * ---------------------------------------------------------------------------------------------- */
int hs_snp_planes(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const uint8_t* d_snp_ref,
                  const uint8_t* d_snp_alt, const int32_t* d_snp_contig, const int64_t* d_contig_snp_base,
                  const int64_t* d_plane_off, const int32_t* d_words, const int32_t* d_n_reads, const int32_t* h_words /* HOST, [C] */,
                  int32_t n_contigs, int32_t n_snps, uint64_t* d_alt, uint64_t* d_ref, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K5 -- read x read similarity / difference.  Replaces list_similarities_and_differences_between_reads3
 * (separate_reads.cpp:374-433): sim = 3*A*At + R*Rt, diff = A*Rt + R*At with zero diagonals, as popcounts of
 * bit-planes. d_alt / d_ref: N rows of `words` uint64 (bit s of row r = read r carries second_base / ref_base
 * at SNP s; a read carries at most one of the two at a SNP: the planes are disjoint, which the kernel relies on). Batched over
 * contigs: plane_off[c] (in uint64 words), out_off[c] (in int32 elements).
 * ---------------------------------------------------------------------------------------------- */
int hs_simdiff(const uint64_t* d_alt, const uint64_t* d_ref, const int64_t* d_plane_off,
               const int32_t* d_n_reads, const int32_t* d_words, const int64_t* d_out_off, int32_t n_contigs,
               int32_t* d_sim, int32_t* d_diff, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K6 -- read graph of every clustering window. Replaces create_read_graph_matrix (separate_reads.cpp:706-828).
 * d_sim / d_diff: the matrices of hs_simdiff, contig c at ctg_out_off[c] with ctg_n_reads[c] rows. A window is
 * (contig, ascending list of its masked read ids); row = one masked read. Output (malloc'ed, release with
 * hs_free_host): nbr_off[rows+1] and nbr = the reads linked to every masked read, ascending (the symmetric adjacency
 * the reference stores in its Eigen matrix / neighbour lists). Rows whose result depends on how std::sort arranges
 * equal distances are finished on the host with std::sort itself; *n_rows_host reports how many.
 * All array arguments except d_sim / d_diff are host pointers.
 * ---------------------------------------------------------------------------------------------- */
int hs_read_graphs(const int32_t* d_sim, const int32_t* d_diff, const int64_t* ctg_out_off, const int32_t* ctg_n_reads,
                   int32_t n_contigs, const int32_t* win_contig, const int64_t* win_mask_off, const int32_t* mask_ids,
                   int32_t n_windows, float error_rate, int64_t** nbr_off, int32_t** nbr, int64_t* n_rows_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A1 -- Myers bit-vector edit distance, batched and banded (64 query rows per lane, carries passed between lanes;
 * a wavefront per pair, queries up to 2048 bases 8 / 16 / 32 lanes per pair; the band's bound is found on the way, as
 * edlib's k = -1 does). The reference's hot path takes base-level alignments from the SAM CIGAR;
 * its bundled edlib (edlib.h:242-246, modes edlib.h:36-62) is the behavioural oracle for this kernel.
 * hs_edit_distance is hs_edlib_align (below) with task DISTANCE and k = -1 for offsets that live on the DEVICE: the same
 * kernels, the same grouping of the pairs, the same scratch budget.
 * mode: 0 = NW (global), 1 = SHW (prefix), 2 = HW (infix). Outputs: edit distance and the first end location
 * on the target (0-based, inclusive), like edlibAlign's editDistance / endLocations[0]. Synchronous with respect to `stream`.
 * ---------------------------------------------------------------------------------------------- */
int hs_edit_distance(const uint8_t* d_query, const int64_t* d_query_off, const uint8_t* d_target,
                     const int64_t* d_target_off, int32_t n_pairs, int32_t mode, int32_t* d_dist,
                     int32_t* d_end, void* stream);

/* A1 as the stage-5 call sites of the reference use their bundled edlib (create_new_contigs.cpp:558-629, tools.cpp:515-534):
 * edlibAlign(query, target, edlibNewAlignConfig(-1, EDLIB_MODE_HW, EDLIB_TASK_PATH, NULL, 0)), batched, one wavefront per
 * pair. d_dist = editDistance, d_end = endLocations[0], d_start = startLocations[0] (edlib.cpp:226-258), d_ops[h_ops_off[i] ..
 * + d_ops_len[i]) = alignment of pair i in edlib's move codes (0 '=', 1 insertion, 2 deletion, 3 mismatch; every pair needs
 * room for query + target operations). d_ops == NULL: locations only (EDLIB_TASK_LOC). d_ops_len[i] = -1 where edlib
 * itself has no alignment to offer (end location -1) or the query has more than 2^20 bases. Long pairs are cut in halves the way
 * edlib cuts them (Hirschberg, edlib.cpp:1166-1404), so the alignment is edlib's at any length. Offsets are HOST arrays [n+1];
 * sequences are base codes 0..3. Synchronous with respect to `stream`. */
int hs_edlib_hw_align(const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off,
                      int32_t n_pairs, int32_t* d_dist, int32_t* d_start, int32_t* d_end, uint8_t* d_ops, const int64_t* h_ops_off,
                      int32_t* d_ops_len, void* stream);

/* edlibAlign(query, target, edlibNewAlignConfig(k, mode, task, NULL, 0)) for n pairs, batched, on the kernels of hs_edlib_hw_align.
 * mode: 0 NW, 1 SHW, 2 HW; task: 0 DISTANCE, 1 LOC, 2 PATH; k = -1 (any k < 0): no bound.
 * d_dist = editDistance (-1 beyond k), d_start / d_end = startLocations[0] / endLocations[0] (-1 when none; no start location
 * for DISTANCE, nor for an empty query or target, as edlib), d_nloc = numLocations (0 beyond k; may be NULL),
 * d_ops / h_ops_off / d_ops_len as hs_edlib_hw_align (task PATH only; may be NULL otherwise; d_ops_len = 0 where edlib has no
 * alignment). With k >= 0 the band of the first sweep is sized from k; a pair within k gets the locations and path of k = -1.
 * Offsets are HOST arrays [n+1]; sequences are codes 0..3. Synchronous with respect to `stream`. */
int hs_edlib_align(const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off,
                   int32_t n_pairs, int32_t mode, int32_t task, int32_t k,
                   int32_t* d_dist, int32_t* d_start, int32_t* d_end, int32_t* d_nloc,
                   uint8_t* d_ops, const int64_t* h_ops_off, int32_t* d_ops_len, void* stream);
/* edlibAlign(query, target, edlibNewAlignConfig(k, mode, task, equalities, n_equalities)) on raw bytes 0..255: any alphabet edlib
 * accepts (up to 256 distinct bytes) with its additionalEqualities (edlib.h:92-95, EqualityDefinition edlib.cpp:61-92: every byte
 * equals itself and the listed pairs are equal both ways; the relation need not be transitive; a pair naming a byte that occurs
 * in neither sequence changes nothing). The bytes the call's sequences hold are compacted to symbols once per call
 * (transformSequences, edlib.cpp:1422-1460) and the equality vectors of a query block (buildPeq, :357-380) come from a table: in
 * LDS up to 16 symbols, in device scratch up to 256; a call with at most four symbols and no equality among them runs on the
 * four-code kernels. h_equalities is a HOST array (NULL / 0: bytes equal themselves only). Outputs, empty-sequence behaviour,
 * error codes and synchronisation as hs_edlib_align; n_equalities < 0, or h_equalities == NULL with n_equalities > 0: HS_EINVAL. */
typedef struct hs_equality_pair { uint8_t first, second; } hs_equality_pair;   /* == EdlibEqualityPair (edlib.h:92-95) */
int hs_edlib_align_bytes(const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off,
                         int32_t n_pairs, int32_t mode, int32_t task, int32_t k,
                         const hs_equality_pair* h_equalities, int32_t n_equalities,
                         int32_t* d_dist, int32_t* d_start, int32_t* d_end, int32_t* d_nloc,
                         uint8_t* d_ops, const int64_t* h_ops_off, int32_t* d_ops_len, void* stream);
/* edlibAlignmentToCigar on host: format 0 STANDARD (M I D), 1 EXTENDED (= X I D); returns a malloc'd string (hs_free_host).
 * An empty alignment gives "". */
int hs_alignment_to_cigar(const uint8_t* ops, int32_t n_ops, int32_t format, char** out);

/* A1 on the path: a CIGAR-less input. The reference reads the base-level alignments from the CIGARs of a SAM file and
 * refuses a .paf (call_variants.cpp:1256-1267; CIGAR required at input_output.cpp:357-368). hs_realign_paf turns a PAF file (read
 * interval, strand, contig interval per line) into that SAM: every read segment is aligned against its contig window (the PAF
 * interval + HS_REALIGN_PAD = 100 bases on both sides) on the device exactly as edlibAlign(segment, window, k = -1, EDLIB_MODE_HW,
 * EDLIB_TASK_PATH) of the reference's bundled edlib aligns it; POS = window start + start location + 1, CIGAR = clips (S) + the
 * path as M / I / D runs, NM:i: = the edit distance, LN:i: = the read length. HS_call_variants takes a .paf this way when
 * HS_REALIGN=1 is set (the SAM goes to <tmpDir>/hs_realigned.sam); without it the reference's refusal stands. */
typedef struct hs_realign_stats { int64_t n_lines, n_aligned, query_bases; double ms_device, ms_total; } hs_realign_stats;
int hs_realign_paf(const char* gfa, const char* reads, const char* paf, const char* out_sam, int32_t n_threads, hs_realign_stats* stats /* may be NULL */);

/* The same input without the two files in between (hs_capi_realign.inc, kernels in hs_kernels_realign.hip): intervals in memory ->
 * a resident hs_cv_batch. The pairs are cut on the device (k_realign_cut), aligned by hs_edlib_hw_align, and the moves it leaves
 * become packed CIGAR words (len << 4 | op, as hs_cv_batch_create takes them) on the device; no move byte crosses to the host.
 *
 * hs_moves_to_cigar -- the kernel-level step: the moves of n pairs exactly as hs_edlib_hw_align leaves them (d_ops + h_ops_off[i],
 * d_ops_len[i]; 0 '=' and 3 mismatch are one class M = 0, 1 is I = 1, 2 is D = 2; any other byte counts as M) -> the words of pair i:
 * clip_left << 4 | 4 if the left clip is > 0, one len << 4 | op per maximal run of one class, clip_right << 4 | 4 if the right clip
 * is > 0, at d_words + d_word_off[i]. A pair with d_ops_len[i] <= 0 gets no words. d_spans[2 i] / [2 i + 1] = M + D / M + I + clips
 * of pair i (the reference and read span hs_cv_batch_create forms from the words). d_words == NULL counts only (offsets, total and
 * spans). Work is split in chunks of 1024 moves, so the number of launches does not depend on n. A pair may hold at most 2^28 - 1
 * moves (the length field of a word). Synchronous with respect to `stream`; HS_EINVAL when d_words != NULL and words_cap < *n_words
 * (nothing is written then). */
int hs_moves_to_cigar(const uint8_t* d_ops, const int64_t* h_ops_off /* [n+1] */, const int32_t* d_ops_len,
                      const int32_t* d_clip_left, const int32_t* d_clip_right /* NULL: no clips */, int32_t n,
                      int64_t* d_word_off /* [n+1] out */, uint32_t* d_words /* NULL: count only */, int64_t words_cap,
                      int32_t* d_spans /* [n][2] reference span, read span; may be NULL */, int64_t* n_words /* host out */, void* stream);

/* hs_realign_intervals -- the job-level step. Interval i says: bases [iv_qstart, iv_qend) of read iv_read lie on bases [iv_tstart,
 * iv_tend) of contig iv_contig, on strand iv_strand (1 forward, 0 reverse: the read segment is reverse-complemented). Each is aligned
 * against contig[max(0, tstart - pad), min(L, tend + pad)) as hs_realign_paf aligns a PAF line; an interval outside its read or
 * contig (qstart < 0, qend > read length, qstart >= qend, and the same on the contig), or naming a read or contig that does not
 * exist, gives HS_EINVAL and hs_last_error() names it. Rounds are bounded by HS_REALIGN_CHUNK_MB as in hs_realign_paf. The records
 * come back grouped by contig (stable: input order inside a contig) in the layout of hs_cv_batch_create, and, when `batch` is not
 * NULL, as a batch made from them. Everything in the result is malloc'ed: release it with hs_realign_records_destroy. */
struct hs_cv_batch;   /* the opaque batch of the stage level below */
typedef struct hs_realign_records {
    int32_t n_intervals, n_rec, n_contigs;
    int32_t* contig_rec_off;   /* [n_contigs+1] */
    int32_t* rec_interval;     /* [n_rec] which input interval; records grouped by contig, input order inside a contig */
    int32_t *rec_read, *rec_pos /* 0-based: window start + start location */, *rec_dist /* NM */;
    uint8_t* rec_strand;       /* 1 forward, 0 reverse: as hs_cv_batch_create */
    int64_t* rec_cig_off; uint32_t* cigar;
    int64_t n_dropped; int32_t* dropped;   /* intervals the aligner had no path for (query > 2^20 bases) */
    double t_cut_ms, t_align_ms, t_cigar_ms, t_download_ms;   /* HIP events / wall around the phases */
    int64_t n_rounds, move_bytes, cigar_words;
    int64_t n_pieces;          /* pairs handed to the aligner (hs_realign_intervals: one per interval) */
    double t_join_ms;          /* hs_realign_intervals_anchored: HIP events around k_anchor_join (0 otherwise) */
} hs_realign_records;
int hs_realign_intervals(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs,
                         const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                         const int32_t* iv_read, const int32_t* iv_contig, const uint8_t* iv_strand,
                         const int32_t* iv_qstart, const int32_t* iv_qend, const int32_t* iv_tstart, const int32_t* iv_tend,
                         int32_t n_intervals, int32_t pad,
                         hs_realign_records** out, struct hs_cv_batch** batch /* may be NULL */);
void hs_realign_records_destroy(hs_realign_records* r);
/* The files of hs_realign_paf (same parser, same refusals, pad = HS_REALIGN_PAD) -> a resident batch, no SAM in between. */
int hs_cv_batch_create_paf(const char* gfa, const char* reads, const char* paf, int32_t n_threads,
                           struct hs_cv_batch** batch, hs_realign_records** recs /* may be NULL */);
/* Its twin for a SAM that exists (the parser of HS_call_variants, then hs_cv_batch_create): what the file route does after hs_realign_paf
 * has written its SAM, and the yardstick `tools/myers_bench.py realign` times hs_cv_batch_create_paf against. */
int hs_cv_batch_create_sam(const char* gfa, const char* reads, const char* sam, int32_t n_threads, struct hs_cv_batch** batch);

/* The two stage-5 computations that sit on those edlib calls, batched (two alignments per item in ONE hs_edlib_hw_align call):
 * hs_reattach_ends == tools.cpp:505-536 (the ends of the backbone that racon dropped are attached to the consensus again),
 * hs_trim_polished == create_new_contigs.cpp:556-629 (the overhangs the piece was polished with are cut off the polished
 * sequence through the alignment path of the piece's ends). Strings are NUL-terminated, at most four distinct bytes per aligned
 * pair (HS_EFORMAT otherwise; the _bytes forms below take any); *out = n malloc'ed strings,
 * released with hs_free_strings. */
int hs_reattach_ends(const char* const* backbone, const char* const* consensus, int32_t n, char*** out);
int hs_trim_polished(const char* const* to_polish, const char* const* newcontig, const int32_t* overhang_left, const int32_t* overhang_right,
                     int32_t n, char*** out);
/* The same two computations (tools.cpp:505-536, create_new_contigs.cpp:556-629) through hs_edlib_align_bytes (HW, k = -1, no
 * equalities, as the reference calls edlib): any bytes -- N runs, soft-masked lower case, IUPAC codes -- compared as edlib
 * compares them. They never refuse an alphabet; everything else as the two calls above. */
int hs_reattach_ends_bytes(const char* const* backbone, const char* const* consensus, int32_t n, char*** out);
int hs_trim_polished_bytes(const char* const* to_polish, const char* const* newcontig, const int32_t* overhang_left,
                           const int32_t* overhang_right, int32_t n, char*** out);
void hs_free_strings(char** s, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Stage level (host buffers in, host buffers out). These run the whole stage exactly as the drop-in
 * executables do: device kernels for pileup / histogram / extraction / sim-diff / Chinese Whispers, host code
 * for the sequential glue. Split in upload + run so callers can time the path with inputs resident in HBM.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_cv_batch hs_cv_batch;   /* opaque: a batch of contigs + reads + records resident in HBM */

/* call_variants.cpp:1249-1262 hand-off: what parse_reads/parse_assembly/parse_SAM produce, flattened. */
int hs_cv_batch_create(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs,
                       const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                       const int32_t* h_rec_read, const int32_t* h_rec_pos, const uint8_t* h_rec_strand,
                       const int64_t* h_rec_cig_off, const uint32_t* h_cigar,
                       const int32_t* h_contig_rec_off, hs_cv_batch** out);
void hs_cv_batch_destroy(hs_cv_batch* b);
/* Optional ploidy of every contig (0 = none), the in-memory counterpart of the <ploidy_of_contigs> file of HS_separate_reads
 * (separate_reads.cpp:1444-1463, used at :1711-1715): the stage-3 -> stage-4 entry points below (hs_sr_run_cv, hs_sr_run_cv_range,
 * hs_pipeline_run) apply it. ploidy == NULL clears it. */
int hs_cv_batch_set_ploidy(hs_cv_batch* b, const int32_t* ploidy /* [n_contigs] or NULL */);
int64_t hs_cv_batch_aligned_bp(const hs_cv_batch* b);   /* number of pileup entries (the metric's unit) */
/* The device the batch lives on (the one that was current on the creating thread). Every entry point that takes a batch binds
 * the calling thread -- and every thread the library starts for it -- to that device first. */
int hs_cv_batch_device(const hs_cv_batch* b);

/* A column of the pileup as the device keeps it between the kernels of stage 3 (16 bytes). */
typedef struct hs_colrec {
    int32_t pos;          /* position on its contig */
    int32_t contig;       /* contig index in the batch */
    uint16_t c0, c1;      /* reads carrying the two most frequent codes (call_variants.cpp:497-507) */
    uint8_t k0, k1;       /* those codes, equal counts in the reference's order (robin_hood iteration order + std::sort) */
    uint8_t flags;        /* HS_COL_* */
    uint8_t c2;           /* the third count, saturating at 63 */
} hs_colrec;
#define HS_COL_CAND 1     /* candidate SNP of call_variants.cpp:525-536 */
#define HS_COL_AUTO 2     /* ... that also passes the automatic threshold (:532) */
#define HS_COL_LOOPD 4    /* may be rescued by loop D (:745-764) */
#define HS_COL_KEEP 8     /* kept by loop C or D */
#define HS_COL_SNP 16     /* in the output (:1335-1352) */
#define HS_COL_TIE 32     /* equal counts among its leading codes */
#define HS_COL_C1GT5C2 64 /* second count > 5 x third count (:526) */

/* Per-contig result of stage 3 == what output_files (call_variants.cpp:1174-1213) prints. */
typedef struct hs_cv_result {
    int32_t n_contigs;
    float* mean_distance;      /* [C] generate_msa's return value */
    float* depth;              /* [C] call_variants.cpp:565 */
    int64_t* snp_off;          /* [C+1] */
    int32_t* snp_pos;          /* [S] */
    uint8_t* snp_ref;          /* [S] */
    uint8_t* snp_alt;          /* [S] */
    int32_t* snp_n_ref;        /* [S] reads carrying snp_ref / snp_alt (what parse_column_file recounts, separate_reads.cpp:151-167) */
    int32_t* snp_n_alt;        /* [S] */
    int64_t* col_off;          /* [S+1] */
    int32_t* col_idx;          /* read indices, ascending */
    uint8_t* col_code;         /* pileup codes */
    float error_rate;          /* call_variants.cpp:1312-1315,1377 */
    int32_t n_contigs_with_error_rate;
    double t_device_ms;        /* wall time of the device phase (uploads of selections, kernels, downloads) */
    double t_host_ms;          /* wall time of the host glue */
    float t_kernel_ms[4];      /* hipEvent time of k_pileup, k_column_stats, k_gather_columns, k_cigar_scan */
    float t_kernel_k4_ms;      /* hipEvent time of k_column_partition_test */
    int64_t n_columns_extracted;        /* K3: columns of the selected positions (they stay on the device) */
    int64_t n_columns_downloaded;       /* of those, candidate SNPs: the columns the host walks (loops A / B) */
    int64_t n_columns_downloaded_late;  /* columns whose leading codes had equal counts (ordered on the device as the reference orders them) */
    int32_t entries_borrowed;           /* col_idx / col_code point into a block of the pipeline that made the result (valid until its next call): not freed with it */
} hs_cv_result;

int hs_cv_run(hs_cv_batch* b, float automatic_snp_threshold, int32_t n_threads, hs_cv_result** out);

/* Test taps of the column pass of stage 3 exactly as the pipeline queues it for the contigs [c0, c1) of a resident batch -- K0, K1, K2
 * (k_column_stats_tiled_dw), k_columns_compact, k_gather_tiles_direct / k_gather_tiles, k_column_top3_exact, k_candidates_scan,
 * k_flag_block_sums / _offsets, k_pack_flagged, k_cand_bits -- with what those kernels left on the device copied out, so that each of
 * them can be held against the oracle on its own (tests/test_gpu_kernels.py). The reference has no counterpart: call_variants.cpp:
 * 471-536 walks positions one by one. */
typedef struct hs_cand_bits {        /* == hs::CandBits (hs_host.h): a candidate column as bit sets over the reads ranked by start position */
    int32_t wlo; uint16_t n_words, n_slots; int32_t idx_min, idx_max, reach, n_entries; int64_t word_off;
} hs_cand_bits;
typedef struct hs_cv_taps {
    int32_t n_contigs;               /* c1 - c0 */
    int64_t n_cols, n_entries;       /* the extracted columns (K2's selection: every position that can still become a SNP) and their entries */
    int64_t* col_gpos;               /* [n_cols] position in the concatenated contigs of the batch, ascending (k_columns_compact) */
    hs_colrec* col_rec;              /* [n_cols] leading codes and counts (K2's second pass / k_column_top3_exact), flags (k_candidates_scan) */
    int64_t* col_off;                /* [n_cols + 1] */
    int32_t* col_idx;                /* [n_entries] read index on the contig, ascending inside a column (k_gather_tiles*) */
    uint8_t* col_code;               /* [n_entries] pileup code */
    int64_t n_cand;                  /* candidates (HS_COL_CAND) */
    hs_colrec* cand_rec;             /* [n_cand] k_pack_flagged: their records ... */
    int32_t* cand_col;               /* ... and their index among the columns */
    hs_cand_bits* cand_bits;         /* [n_cand] k_cand_bits */
    uint64_t* cand_words;            /* [n_cand_words] */
    int64_t n_cand_words;
    int32_t* contig_n_cand;          /* [n_contigs] */
    float* contig_mean_distance;     /* [n_contigs] k_contig_error */
} hs_cv_taps;
int hs_cv_column_pass_taps(hs_cv_batch* b, int32_t c0, int32_t c1, float automatic_snp_threshold, hs_cv_taps** out);
void hs_cv_taps_destroy(hs_cv_taps* t);

/* Test tap of the pileup as a contig group of the pipeline launches it: K0 + K1 (+ the records K0 flagged) of the contigs [c0, c1) on the resident
 * batch's own pile layout (every record at an address = contig_off + pos mod 128) and its own prebuilt task slice. Before the launch the WHOLE pile
 * allocation -- the bytes in front of the first record, every record, every gap, the bytes behind the last -- is set to the byte `fill`, and the batch's
 * rec_stats and chunk table to 0xFF bytes, so that every byte a kernel writes outside its records, or outside the range, shows. Host copies of what the
 * device holds afterwards. No kernel of its own, nothing on the product path. */
typedef struct hs_cv_pileup_taps {
    int32_t n_rec;
    int32_t pile_lead;               /* bytes of the allocation in front of the pile's byte 0 (what pile_addr counts from) */
    int64_t pile_alloc_bytes;        /* pile_lead + pile_addr[n_rec] + the bytes behind */
    int64_t n_chunks;                /* rec_chunk_off[n_rec] */
    uint8_t* pile;                   /* [pile_alloc_bytes] the whole allocation */
    int64_t* pile_addr;              /* [n_rec + 1] */
    int32_t* rec_stats;              /* [n_rec][4] q_end, n_err, n_len, events */
    int64_t* rec_chunk_off;          /* [n_rec + 1] */
    int32_t* chunk_table;            /* [n_chunks][4] K0's table */
} hs_cv_pileup_taps;
int hs_cv_pileup_tap(hs_cv_batch* b, int32_t c0, int32_t c1, int32_t fill, hs_cv_pileup_taps** out);
void hs_cv_pileup_tap_destroy(hs_cv_pileup_taps* t);

/* Several GPUs in one process. Contigs are the independent units of both stages (call_variants.cpp:1276-1280,
 * separate_reads.cpp:1506-1508): hs_cv_run_host and hs_sr_run shard them over the devices of hs_devices() by
 * longest-processing-time (stage 3: bases of the reads aligned to the contig; stage 4: N^2 + N * S), one host thread and one
 * device per shard, results merged in contig order (the error rate over the whole job). hs_devices: the device list =
 * HS_DEVICES="0,1,.." or every visible device; a device may be listed more than once (two shards on one GPU).
 * hs_cv_run_host = hs_cv_batch_create + hs_cv_run + destroy per shard (host buffers as for hs_cv_batch_create). */
int hs_devices(int32_t* out, int32_t cap);       /* returns the number of devices of the list */
int hs_cv_run_host(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs,
                   const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                   const int32_t* h_rec_read, const int32_t* h_rec_pos, const uint8_t* h_rec_strand,
                   const int64_t* h_rec_cig_off, const uint32_t* h_cigar, const int32_t* h_contig_rec_off,
                   float automatic_snp_threshold, int32_t n_threads, hs_cv_result** out);

/* hs_cv_run in two steps, for hosts that overlap the sequential glue of several contig groups:
 * hs_cv_select = the streaming pass over the WHOLE batch (K0 CIGAR scan, K1 pileup, K2 column statistics; one launch each),
 * hs_cv_run_range = everything after it (K3, partitions, K4, merge) for the contigs [c0, c1) of the batch. Contigs are
 * independent (call_variants.cpp:1280): ranges may run concurrently from different host threads; the result of a range
 * holds c1 - c0 contigs and its error_rate covers that range only (form the job-wide mean from mean_distance). */
typedef struct hs_cv_selection {
    int64_t n_selected;        /* positions whose second allele count makes them worth extracting */
    float t_kernel_ms[4];      /* hipEvent time of k_pileup, k_column_stats, -, k_cigar_scan */
    double t_device_ms, t_host_ms;
    void* impl;
} hs_cv_selection;
int hs_cv_select(hs_cv_batch* b, hs_cv_selection** out);
int hs_cv_run_range(hs_cv_batch* b, const hs_cv_selection* sel, int32_t c0, int32_t c1, float automatic_snp_threshold,
                    int32_t n_threads, hs_cv_result** out);
void hs_cv_selection_destroy(hs_cv_selection* sel);
void hs_cv_result_destroy(hs_cv_result* r);

/* Stage 4 on SNP columns already in memory (what parse_column_file, separate_reads.cpp:46-190, yields). */
typedef struct hs_sr_contig {
    int64_t length;            /* contig length */
    int32_t n_reads;           /* number of READ lines */
    const int32_t* read_start; /* [n_reads] readLimits .first */
    const int32_t* read_end;   /* [n_reads] readLimits .second */
    int32_t n_snps;
    const int32_t* snp_pos;
    const uint8_t* snp_ref;
    const uint8_t* snp_alt;
    const int64_t* col_off;    /* [n_snps+1] offsets into col_idx / col_code (need not start at 0) */
    const int32_t* col_idx;
    const uint8_t* col_code;
    int32_t ploidy;            /* 0 = unlimited (separate_reads.cpp:1454-1458) */
} hs_sr_contig;

typedef struct hs_sr_result {
    int32_t n_contigs;
    int64_t* win_off;          /* [C+1] windows per contig */
    int32_t* win_start;        /* [W] */
    int32_t* win_end;          /* [W] */
    int64_t* label_off;        /* [W+1] offsets into labels (n_reads of the contig each) */
    int32_t* labels;           /* -2 absent, -1 unclustered, >=0 group */
    double t_device_ms;
    double t_host_ms;
    int64_t n_cw_instances;
    float t_kernel_ms[4];      /* hipEvent time of k_simdiff and of the three k_chinese_whispers waves */
    float t_kernel_graph_ms;   /* hipEvent time of k_read_graph_rows */
    int64_t n_graph_rows_host; /* graph rows whose neighbour cut-off depended on std::sort's order of equal keys */
    int64_t n_windows_finished_on_host;   /* clustering windows whose cluster merging (K8) fell back to the host code */
    /* counts behind the whole-path roofline of SURVEY.md 8(d): emitted by the kernels / the driver, not estimated */
    int64_t n_cw_sweeps;       /* Chinese-Whispers sweeps, summed over every run */
    int64_t cw_bytes;          /* sum over runs of sweeps * (4 * nnz + 8 * m), nnz / m = neighbour entries / nodes of the run's window graph */
    int64_t graph_nnz;         /* neighbour entries of all window graphs */
    int64_t n_graph_rows;      /* rows (window, masked read) of all window graphs */
    int64_t simdiff_bytes;     /* sum over matrix-path contigs of N * S / 4 + 16 * N * N */
} hs_sr_result;

int hs_sr_run(const hs_sr_contig* contigs, int32_t n_contigs, int32_t window_size, float error_rate,
              int32_t low_memory, uint32_t seed, int32_t n_threads, hs_sr_result** out);

/* Test taps of the clustering chain of stage 4 exactly as hs_sr_run queues it: for every window that has seeding SNPs (chain order) its
 * contig, first position and reads, and what the kernels of the chain left -- the labels of every per-SNP Chinese-Whispers run
 * (separate_reads.cpp:1674-1705: k_cw_seed_sets + k_cw_seeded_lanes / k_cw_seeded_rows / k_cw_seeded_wave) as READ indices, and the labels of
 * the run behind finalize_clustering's small-cluster filter (:924-970, inside k_window_tail). The finished labels are in the result. */
typedef struct hs_sr_taps {
    int32_t n_windows;
    int32_t* win_contig; int32_t* win_start;      /* [n_windows] */
    int64_t* win_row0;                            /* [n_windows + 1] into mask_ids / third */
    int32_t* mask_ids;                            /* the window's reads, ascending */
    int64_t* run_begin;                           /* [n_windows + 1] the window's per-SNP runs */
    int32_t* run_snp;                             /* SNP index on its contig of every run */
    int64_t* run_off;                             /* [runs + 1] into run_labels: m labels per run, in the order of mask_ids */
    int32_t* run_labels;                          /* label = the read index the label stands for */
    int32_t* third;                               /* cluster index (-1: dropped with its small cluster) */
    /* mode HS_SR_TAPS_GRAPHS: the fields above stay empty; the front of the call as its kernels left it, reached through the calls hs_sr_run makes
     * (K5a k_snp_planes, K5 k_simdiff, k_simdiff_windows, K6 k_read_graph_rows and the row fetch, patch, degree and fill kernels) */
    int32_t g_n_windows;                          /* EVERY window of the call's window set, in set order */
    int32_t* g_win_contig; int32_t* g_win_kind;   /* kind: 0 = graph from the contig's sim / diff matrices, 1 = low-memory path on the device, 2 = on the host */
    int64_t* g_win_row0;                          /* [g_n_windows + 1] into g_mask_ids / g_nbr_off */
    int32_t* g_mask_ids;                          /* the window's reads, ascending */
    int64_t* g_nbr_off; int32_t* g_nbr;           /* [rows + 1]; the neighbours of every (window, read) row as READ indices, ascending */
    int32_t g_n_contigs;
    int32_t* g_plane_n; int32_t* g_words;         /* [C] reads / 64-SNP words of the contig's bit rows (0: it has none) */
    int64_t* g_plane_off;                         /* [C] first word of the contig in g_alt / g_ref; word w of read r at plane_off + r * words + w */
    uint64_t* g_alt; uint64_t* g_ref;             /* the bit rows as K5a left them (every word is stored by K5a: the buffers are all ones before it) */
    int32_t* g_n_reads; int64_t* g_out_off;       /* [C] reads of the contig's matrices (0: none) / its first pair in g_matrix */
    int64_t* g_read_base; int32_t* g_pos_orig;    /* row k of the matrices of contig c is the read g_pos_orig[g_read_base[c] + k] (reads by start position) */
    int64_t g_n_pos_orig, g_n_plane_words, g_n_pairs;
    int32_t* g_matrix;                            /* (sim, diff) of rows (i, j) at 2 * (out_off + i * n_reads + j); HS_SR_TAP_SENTINEL in both: K5 did not write
                                                     the pair (a tile of two 64-row blocks that share no SNP word: nobody reads it) */
    int64_t g_rows_on_host, g_rows_late;          /* rows resolved on the host / of those, fetched behind the row kernels (no room in the staging area) */
    int32_t g_row_waves;                          /* wavefronts per workgroup of k_read_graph_rows (4, or 1 for a window wider than 1792 reads; 0: not launched) */
    /* mode HS_SR_TAPS_CHAIN: the routes the chain took, from the lists the call builds on the host (and the overflow list's length on the device) */
    int32_t all_lanes;                            /* 1: every chain window had at most 64 reads (the host branch of its own for that case) */
    int32_t cap_tail;                             /* nodes the LDS of k_window_tail holds in this call (at most 2048) */
    int64_t runs_lanes, runs_overflow;            /* per-SNP runs one per lane (k_cw_seeded_lanes); of those, runs with more than 16 labels alive: one wavefront each */
    int64_t runs_rows, units_rows;                /* runs of k_cw_seeded_rows (windows of 65 .. 255 reads) / its units of up to eight runs */
    int64_t runs_wave, runs_wave_scratch;         /* runs of k_cw_seeded_wave (more than 255 reads) / of those, with their nodes in global scratch */
    int64_t tail_narrow, tail_lds, tail_scratch;  /* windows of k_window_tail with labels in registers (at most 64 reads) / LDS / global scratch (more than cap_tail) */
} hs_sr_taps;
#define HS_SR_TAPS_CHAIN 0
#define HS_SR_TAPS_GRAPHS 1                       /* stops behind the read graphs: no Chinese-Whispers chain, *out stays NULL */
#define HS_SR_TAP_SENTINEL INT32_MIN              /* the matrices are filled with it before K5, in this mode only (the one extra launch of the taps) */
int hs_sr_run_taps(const hs_sr_contig* contigs, int32_t n_contigs, int32_t window_size, float error_rate, int32_t low_memory, uint32_t seed,
                   int32_t n_threads, int32_t mode, hs_sr_result** out, hs_sr_taps** taps);
void hs_sr_taps_destroy(hs_sr_taps* t);
void hs_sr_result_destroy(hs_sr_result* r);
/* Stage 4 directly on the result of hs_cv_run, without the .col text round trip (call_variants.cpp:1197-1204 <->
 * separate_reads.cpp:84-170). READ limits come from the records (input_output.cpp:503-511); SNPs whose second base is
 * rarer than rarest_strain_abundance are dropped as parse_column_file does (separate_reads.cpp:167). window_size <= 0:
 * computed as separate_reads.cpp:1466-1498 from this batch. */
int hs_sr_run_cv_range(const hs_cv_batch* b, int32_t c0, int32_t c1, const hs_cv_result* cv, float error_rate,
                       float rarest_strain_abundance, int32_t low_memory, int32_t amplicon, uint32_t seed, int32_t n_threads,
                       int32_t window_size, hs_sr_result** out);   /* cv = result of hs_cv_run_range(b, sel, c0, c1) */
int hs_sr_run_cv(const hs_cv_batch* b, const hs_cv_result* cv, float error_rate, float rarest_strain_abundance,
                 int32_t low_memory, int32_t amplicon, uint32_t seed, int32_t n_threads, int32_t window_size,
                 hs_sr_result** out);
/* separate_reads.cpp:1466-1498: window size from the read limits of all contigs of the .col */

/* ------------------------------------------------------------------------------------------------
 * Per-group allele calls at every SNP: the finished labels of stage 4 crossed with the SNP columns of stage 3, on the device.
 * The reference forms the same majority base per intermediate cluster and SNP inside merge_wrongly_split_haplotypes
 * (separate_reads.cpp:1056-1113) and discards it; here it is formed on the FINAL labels and returned.
 * A cell = (window, SNP column, group). The groups of a window are its distinct labels >= 0, ascending (ids are kept as they are). A window's
 * SNPs are the columns with win_start <= pos <= win_end; windows without SNPs, and SNPs in no window, are not in the table. Over the
 * column entries whose read has the group's label in that window (entries labelled -1 / -2 count nowhere): n = their number; best /
 * second = the largest and second-largest count of one pileup code (two codes tied at the top: second == best); best_code = the smallest
 * code with the count best; n_ref / n_alt = entries equal to the column's snp_ref / snp_alt; call = best_code, or 0 (undefined) when
 * 2 * second > best or n > 2 * best -- secondMax*2 > max || nb*0.5 > max of separate_reads.cpp:1100 -- or the group has no entry.
 * n_calls of a SNP = distinct non-zero calls among its groups (maxbases.size() of separate_reads.cpp:1113); >= 2: the SNP separates groups.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_allele_cell { uint16_t n, best, second, n_ref, n_alt; uint8_t best_code, call; } hs_allele_cell;   /* 12 bytes */
typedef struct hs_allele_table {   /* separate_reads.cpp:1056-1113; host memory, CSR; release with hs_allele_table_destroy */
    int64_t n_windows, n_snps, n_groups, n_cells;
    int32_t *win_contig, *win_start, *win_end;   /* [n_windows] the windows that have SNPs, contig order */
    int64_t* win_group_off;                      /* [n_windows + 1] into group_ids */
    int32_t* group_ids;                          /* [n_groups] ascending inside a window */
    int64_t* win_snp_off;                        /* [n_windows + 1] the window's SNPs */
    int32_t *snp_contig, *snp_pos;               /* [n_snps] */
    uint8_t *snp_ref, *snp_alt;                  /* [n_snps] pileup codes */
    int32_t* snp_n_calls;                        /* [n_snps] */
    int64_t* snp_cell_off;                       /* [n_snps + 1]: cell of group k of the SNP's window at cells[snp_cell_off[s] + k] */
    hs_allele_cell* cells;                       /* [n_cells] */
    double t_kernel_ms;                          /* hipEvent time of the kernels (0 on an untimed step) */
    int64_t n_entries;                           /* column entries the cell kernels read (5 bytes each) */
    int64_t n_wide_columns;                      /* columns deeper than hs_alleles_lds_capacity(): sorted in global scratch */
} hs_allele_table;
void hs_allele_table_destroy(hs_allele_table* t);   /* separate_reads.cpp:1056-1113 has no such result to release: it discards it */
/* <outfile>.alleles.tsv of HS_separate_reads under HS_ALLELES=1 (separate_reads.cpp:1056-1113 prints nothing): per window
 * "WINDOW <contig> <start> <end> <group ids,>", then per SNP "SNP <pos> <ref base> <alt base> <n_calls>" and per group
 * "g:n:n_ref:n_alt:call", tab-separated; call = the three-base context of the code (call_variants.cpp:25-31) or "."; names[c] = name of
 * contig c (NULL: indices). *out is malloc'ed: hs_free_host. */
int hs_alleles_text(const hs_allele_table* t, const char* const* names, int32_t n_names, char** out);
/* Entries of the deepest column whose keys one wavefront sorts in LDS; deeper columns (up to 65535 entries) go through global scratch. */
int32_t hs_alleles_lds_capacity(void);
/* The kernel-level call (separate_reads.cpp:1056-1113 per cluster -> per final group), asynchronous on `stream`, in two steps that share
 * d_work (hs_group_alleles_layout: byte offsets of its parts; total_bytes to allocate, 256-byte aligned):
 *   d_cells == NULL: the plan -- snp_win [S] (window of every SNP, -1 none), grp_n [W] / grp_ids (the groups of window w at grp_ids +
 *     label_off[w]; windows without SNPs get none), grp_off [W + 1] / grp_pack (the same lists one after the other),
 *     win_snp_first / win_snp_last [W] (SNP range; first == last: none), cell_off [S + 1] (cell_off[S] = cells needed);
 *   d_cells != NULL: the cells of that plan into d_cells (a column whose cells would end beyond cells_cap is not written and gets
 *     n_calls = -1), n_calls [S].
 * Columns: CSR over all SNPs (d_col_off [S + 1], d_col_idx = read index on its contig, d_col_code), at most 65535 entries each; per SNP
 * ref / alt code, position and contig; windows of contig c = [d_win_off[c], d_win_off[c + 1]), ascending; labels of window w =
 * d_labels[d_label_off[w] ...], one per read of its contig (-2 absent, -1 unclustered, >= 0 group; ids below INT32_MAX). */
typedef struct hs_allele_layout { int64_t snp_win, grp_n, win_snp_first, win_snp_last, cell_off, grp_off, n_calls, grp_ids, grp_pack, internal, total_bytes; } hs_allele_layout;
int hs_group_alleles_layout(int32_t n_snps, int32_t n_windows, int64_t n_labels, hs_allele_layout* out);
int hs_group_alleles(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code,
                     const uint8_t* d_snp_ref, const uint8_t* d_snp_alt, const int32_t* d_snp_pos, const int32_t* d_snp_contig, int32_t n_snps,
                     const int64_t* d_win_off /* [n_contigs + 1] */, const int32_t* d_win_start, const int32_t* d_win_end, int32_t n_contigs, int32_t n_windows,
                     const int64_t* d_label_off /* [n_windows + 1] */, const int32_t* d_labels, int64_t n_labels,
                     void* d_work, hs_allele_cell* d_cells, int64_t cells_cap, void* stream);
/* The stage-level call (separate_reads.cpp:1056-1113 on the final labels): the contigs hs_sr_run takes and a result with dense labels --
 * its own, or any labels in that layout. SNP positions must ascend on every contig. */
int hs_haplotype_alleles(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr_result, hs_allele_table** table);

/* ------------------------------------------------------------------------------------------------
 * A window's unlabelled reads recruited to its groups: stage 4 labels only the reads present at a window's first AND last SNP
 * (separate_reads.cpp:1590-1622); every other read that crosses the window is -2 there, and the reads of clusters below the size filter
 * are -1 (separate_reads.cpp:938). Such a read still carries alleles at some of the window's SNPs; here they are held against the calls
 * of the allele table (separate_reads.cpp:1056-1113 on the final labels), on the device that holds both.
 * Windows, SNPs, groups and cells are exactly the allele table's. A ROW is a pair (window w, read r) where r has at least one entry in a
 * SNP column of w (0 <= r < n_reads of the contig; other indices are ignored) and r's label in w is selected by `which`:
 * HS_RECRUIT_ABSENT -2, HS_RECRUIT_UNCLUSTERED -1, HS_RECRUIT_LABELLED >= 0 (evaluation rows: they never change a label). A window with
 * SNPs but no group has no rows; a read in two windows has two independent rows. Rows are window-major, reads ascending.
 * For group k of w, over every entry (r, code) of r in a column s of w, duplicates counted: call(s, k) == 0: not counted for k;
 * code == call(s, k): a match (m_k); any other code: a mismatch (x_k). Any of the 125 codes can match. Counters are 32-bit; n_entries =
 * the read's entries in the window's columns. score_k = m_k - x_k, signed. best = the group of largest score, the smallest id among equal
 * scores; second = the same among the others (one group: -1, counts 0). assigned iff (a) m_best + x_best >= min_informative, (b) one group
 * or score_best - score_second >= min_margin, (c) x_best * mismatch_den <= mismatch_num * (m_best + x_best), in 64 bits.
 * ---------------------------------------------------------------------------------------------- */
#define HS_RECRUIT_ABSENT 1
#define HS_RECRUIT_UNCLUSTERED 2
#define HS_RECRUIT_LABELLED 4
/* separate_reads.cpp:1590-1622, 938, 1056-1113. Refused with HS_EINVAL unless min_informative >= 1, min_margin >= 1 (equal scores never
 * assign), mismatch_den >= 1 and 0 <= mismatch_num <= mismatch_den. */
typedef struct hs_recruit_params { int32_t which, min_informative, min_margin, mismatch_num, mismatch_den; } hs_recruit_params;
/* which = ABSENT | UNCLUSTERED, min_informative 3, min_margin 2, mismatch 1/4. These defaults are PLACEHOLDERS of the interface: nobody
 * has validated or tuned them (separate_reads.cpp:1590-1622, 938, 1056-1113 has no such step to take figures from). */
hs_recruit_params hs_recruit_params_default(void);
/* separate_reads.cpp:1590-1622, 938, 1056-1113: one row; groups as ids, -1 = none. 40 bytes. */
typedef struct hs_recruit_row {
    int32_t read, label, best_group, second_group;
    uint32_t m_best, x_best, m_second, x_second, n_entries;
    int32_t assigned;
} hs_recruit_row;
typedef struct hs_recruit_table {   /* separate_reads.cpp:1590-1622, 938, 1056-1113; host memory; release with hs_recruit_table_destroy */
    int64_t n_windows, n_rows, n_assigned;
    int32_t *win_contig, *win_start, *win_end;   /* [n_windows] the allele table's windows (those that have SNPs), same order */
    int64_t* win_index;                          /* [n_windows] the window's index among ALL windows of the call (label_off of its result) */
    int64_t* win_row_off;                        /* [n_windows + 1] into rows */
    hs_recruit_row* rows;                        /* [n_rows] */
    hs_recruit_params params;                    /* the thresholds used */
    int64_t n_call_windows;                      /* all windows of the call, with or without SNPs */
    int64_t n_counter_words;                     /* 32-bit counters the kernels kept: 1 + 2 * groups per row */
    int64_t n_entries;                           /* column entries the count kernel read */
    double t_kernel_ms;                          /* hipEvent time of the recruit kernels alone (0 on an untimed step) */
} hs_recruit_table;
void hs_recruit_table_destroy(hs_recruit_table* t);   /* separate_reads.cpp:1590-1622, 938, 1056-1113 */
/* The stage-level call (separate_reads.cpp:1590-1622, 938, 1056-1113), twin of hs_haplotype_alleles with the same input rules. params ==
 * NULL: the defaults. alleles may be NULL; otherwise *alleles receives the allele table of the same call. On an error *out stays NULL. */
int hs_recruit_reads(const hs_sr_contig* contigs, int32_t n_contigs, const hs_sr_result* sr_result, const hs_recruit_params* params,
                     hs_allele_table** alleles, hs_recruit_table** out);
/* The kernel-level call (separate_reads.cpp:1590-1622, 938, 1056-1113), twin of hs_group_alleles with the same inputs, asynchronous on
 * `stream`, in two steps over d_work (hs_group_recruit_layout; the allele plan lies at its front, `alleles` gives its parts):
 *   d_cells == NULL: the allele plan, then `flag` [n_labels] (1 = the read's slot of the dense label layout is a row), `row_idx`
 *     [n_labels + 1] (row of every flagged slot; row_idx[n_labels] = rows) and `ctr_off` [n_labels + 1] (first counter word of every
 *     flagged slot; ctr_off[n_labels] = 32-bit words to make room for in d_counters);
 *   d_cells != NULL: the cells, then the counters and d_rows [rows], `win_row_off` [n_windows + 1] over all windows of the call. Nothing
 *     is written beyond rows_cap rows or counters_cap words; `status` is 0, or 1 when either did not suffice. */
typedef struct hs_recruit_layout { hs_allele_layout alleles; int64_t flag, row_idx, ctr_off, win_row_off, status, internal, total_bytes; } hs_recruit_layout;
int hs_group_recruit_layout(int32_t n_snps, int32_t n_windows, int64_t n_labels, hs_recruit_layout* out);
int hs_group_recruit(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code,
                     const uint8_t* d_snp_ref, const uint8_t* d_snp_alt, const int32_t* d_snp_pos, const int32_t* d_snp_contig, int32_t n_snps,
                     const int64_t* d_win_off, const int32_t* d_win_start, const int32_t* d_win_end, int32_t n_contigs, int32_t n_windows,
                     const int64_t* d_label_off, const int32_t* d_labels, int64_t n_labels, const hs_recruit_params* params,
                     void* d_work, hs_allele_cell* d_cells, int64_t cells_cap, uint32_t* d_counters, int64_t counters_cap,
                     hs_recruit_row* d_rows, int64_t rows_cap, void* stream);
/* Device-free (separate_reads.cpp:1590-1622, 938, 1056-1113): labels_out = labels_in, except that every assigned row whose old label is
 * < 0 gets its best_group. label_off: of the result the table was formed on ([n_call_windows + 1]); LABELLED rows never change anything. */
int hs_recruit_apply(const hs_recruit_table* table, const int64_t* label_off, const int32_t* labels_in, int32_t* labels_out, int64_t n_labels);
/* <outfile>.recruit.tsv of HS_separate_reads under HS_RECRUIT=1 (separate_reads.cpp:1590-1622, 938, 1056-1113 prints nothing): per window
 * "WINDOW <contig> <start> <end>", then per row "READ <index> <label> <best> <m> <x> <second> <m2> <x2> <n_entries> <0|1>", tab-separated.
 * names[c] = name of contig c (NULL: indices). *out is malloc'ed: hs_free_host. */
int hs_recruit_text(const hs_recruit_table* t, const char* const* names, int32_t n_names, char** out);

/* ------------------------------------------------------------------------------------------------
 * Both stages over one resident batch with the contigs processed as n_groups consecutive ranges on persistent host threads
 * (one HIP stream and one worker pool each). hs_pipeline_select runs hs_cv_select (the streaming kernels, once over the whole
 * batch) and returns the per-contig mean distances, which only need K1's per-record counters; the caller forms the error
 * rate from them (job-wide, contig order, call_variants.cpp:1312-1315,1377 -- across processes if the job is sharded);
 * hs_pipeline_run then takes every group through hs_cv_run_range and hs_sr_run_cv_range back to back, no barrier between the
 * stages, and concatenates the results in contig order. Equivalent to hs_cv_run + hs_sr_run_cv on the whole batch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_pipeline hs_pipeline;
typedef struct hs_pipeline_stats {
    int64_t n_snps, n_cw_instances, n_graph_rows_host;
    double t_device_ms, t_host_ms;      /* summed over the groups */
    float t_kernel_cv_ms[4];            /* k_pileup, k_column_stats, k_gather_columns (+top3), k_cigar_scan */
    float t_kernel_k4_ms;
    float t_kernel_sr_ms[4];            /* k_simdiff and the three k_chinese_whispers waves */
    float t_kernel_graph_ms;
    int64_t n_columns_extracted, n_columns_downloaded, n_columns_downloaded_late;   /* see hs_cv_result */
    int64_t n_cw_sweeps, cw_bytes, graph_nnz, n_graph_rows, simdiff_bytes;          /* see hs_sr_result */
} hs_pipeline_stats;
int hs_pipeline_create(hs_cv_batch* b, int32_t n_groups, hs_pipeline** out);
int hs_pipeline_select(hs_pipeline* p, float* mean_distance /* [C] out */, hs_pipeline_stats* stats);
/* window_size <= 0: chosen over the whole batch as separate_reads.cpp:1466-1498 does over the whole .col file */
int hs_pipeline_run(hs_pipeline* p, float automatic_snp_threshold, float error_rate, float rarest_strain_abundance, int32_t low_memory,
                    int32_t amplicon, uint32_t seed, int32_t n_threads, int32_t window_size, hs_sr_result** out,
                    hs_pipeline_stats* stats);
/* hs_pipeline_select + the job-wide error rate + hs_pipeline_run in one call, for a job that lives in ONE process: every contig
 * group brings up its own share of the pileup (one group at a time), the error rate (call_variants.cpp:1312-1315, then %g and
 * the 0.15 cap of hairsplitter.py:686-692,725) is formed inside when the last group has its counters. mean_distance
 * [n_contigs] and error_rate_out are optional outputs. Same results as the two calls. */
int hs_pipeline_run_fused(hs_pipeline* p, float automatic_snp_threshold, float rarest_strain_abundance, int32_t low_memory, int32_t amplicon,
                          uint32_t seed, int32_t n_threads, int32_t window_size, float* mean_distance, float* error_rate_out, hs_sr_result** out,
                          hs_pipeline_stats* st);
/* the HIP device each contig-group thread of the pipeline is bound to (== hs_cv_batch_device of its batch); returns the number
 * of groups, fills at most cap entries */
int hs_pipeline_thread_devices(hs_pipeline* p, int32_t* out, int32_t cap);
/* What a pipeline call leaves with the host besides the labels. Stage 3's SNP columns are handed to stage 4 on the device; with
 * HS_PIPELINE_KEEP_COLUMNS != 0 their entries (.col's payload: read indices and codes of every SNP column, the SNPS lines of
 * call_variants.cpp:1184-1204) are ALSO brought to the host inside the call, and the groups' stage-3 results stay available through
 * hs_pipeline_group_cv until the next call on the pipeline (they are dropped when it starts; their col_idx / col_code point into pinned
 * blocks of the pipeline -- hs_cv_result::entries_borrowed -- and are not the caller's to free). Default 0: positions, alleles and
 * counts of the SNPs only. */
#define HS_PIPELINE_KEEP_COLUMNS 1
/* HS_PIPELINE_SPARSE_LABELS != 0: the labels come back per window as the reads the window holds and their labels -- what the GROUP lines
 * of the .gro list (separate_reads.cpp:1756-1784), nothing else: hs_sr_result::labels is NULL (label_off still describes the dense
 * form) and hs_pipeline_sparse_labels returns, valid until the next call on the pipeline, win_row_off [W+1], ids [rows] (ascending
 * read indices inside a window) and labels [rows]; every read a window does not list has the label -2. */
#define HS_PIPELINE_SPARSE_LABELS 2
/* HS_PIPELINE_ALLELES != 0: every contig group also forms its share of the allele table (separate_reads.cpp:1056-1113 on the final labels)
 * at the end of its own chain, from the SNP columns where stage 4 read them on the device -- HS_PIPELINE_KEEP_COLUMNS is not needed -- and
 * hs_pipeline_alleles returns the call's table, contig order, valid until the next call on the pipeline. Off (the default): no launch and
 * no wait is added to the step. */
#define HS_PIPELINE_ALLELES 4
const hs_allele_table* hs_pipeline_alleles(const hs_pipeline* p);   /* NULL before the first call with HS_PIPELINE_ALLELES */
/* HS_PIPELINE_RECRUIT != 0: every contig group also recruits its windows' unlabelled reads (separate_reads.cpp:1590-1622, 938, 1056-1113;
 * hs_recruit_table above) behind its allele cells, from the dense labels that share uploads, in the two host waits it makes anyway. It
 * implies the cells on the device; the allele table itself is exposed only if HS_PIPELINE_ALLELES is set too. hs_pipeline_recruits returns
 * the call's table, contig order, valid until the next call. Thresholds: hs_pipeline_set_recruit_params (HS_EINVAL for a refused set; the
 * defaults until then). Off (the default): no launch, allocation or wait is added to the step. */
#define HS_PIPELINE_RECRUIT 8
const hs_recruit_table* hs_pipeline_recruits(const hs_pipeline* p);   /* NULL before the first call with HS_PIPELINE_RECRUIT */
int hs_pipeline_set_recruit_params(hs_pipeline* p, const hs_recruit_params* params);
int hs_pipeline_set_option(hs_pipeline* p, int32_t option, int64_t value);
int hs_pipeline_groups(const hs_pipeline* p);                                  /* number of contig groups */
int hs_pipeline_group_range(const hs_pipeline* p, int32_t g, int32_t* c0, int32_t* c1);   /* contigs [c0, c1) of group g */
int hs_pipeline_sparse_labels(const hs_pipeline* p, const int64_t** win_row_off, const int32_t** ids, const int32_t** labels, int64_t* n_windows, int64_t* n_rows);
const hs_cv_result* hs_pipeline_group_cv(const hs_pipeline* p, int32_t g);    /* stage-3 result of group g from the last call (NULL before the first) */
void hs_pipeline_destroy(hs_pipeline* p);

int32_t hs_sr_window_size(const hs_sr_contig* contigs, int32_t n_contigs, int32_t amplicon);

/* File-level entry points == main() of the two reference executables (same argv, same exit codes).
 * call_variants.cpp:1215-1385 and separate_reads.cpp:1398-1790. */
int hs_call_variants_main(int argc, char** argv);
/* What HS_call_variants may still do once hs_call_variants_main has returned 0 and its outputs are complete: stage 4 for the arguments
 * hairsplitter.py passes by default (hairsplitter.py:686-692,725-726), in the process that still holds the job's device state; the
 * .gro is left as <out.col>.hsgro and hs_separate_reads_main copies it ONLY if it is called with that .col (size and block hashes
 * of the .hsbin companion) and exactly those arguments (error rate, rarest strain abundance 0.01, low memory 0, the same amplicon
 * switch, HS_SEED, no ploidies); anything else runs stage 4 as always. The executable calls it after it has reported its exit
 * status (csrc/hs_dropin_main.h). HS_NO_PRECOMPUTE=1: neither written nor read. No-op without a preceding successful main. */
void hs_call_variants_epilogue(void);
int hs_separate_reads_main(int argc, char** argv);
/* for executables that _exit right after one of the two: nothing is torn down at the end (parsed inputs, results, device state) */
void hs_main_process_exits(int yes);

/* ------------------------------------------------------------------------------------------------
 * Next stage, consumer side of the .gro (host code, no device work): how every read threads through the contigs that the
 * read separation implies, as a GAF.  Replaces parse_split_file + merge_intervals (+ stitch) + find_paths + output_GAF
 * (create_new_contigs.cpp:41-175, :1427-1534, :833-903, :959-1112, :1128-1419) as called from its main (:1582-1590).
 * hs_gaf_from_files reads the same four files the reference's HS_create_new_contigs reads; hs_gaf_from_labels takes the
 * windows and labels of an hs_sr_result instead of the .gro text (contig_has_snps[c] = 0 for the contigs the .gro writer
 * skips, separate_reads.cpp:1522-1524; NULL = the contigs without windows, which is what hs_sr_run leaves them with).  hs_gro_to_gaf_main: argv = <gfa> <reads> <sam> <gro> <amplicon> <out.gaf> [threads].
 * ---------------------------------------------------------------------------------------------- */
int hs_gaf_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t amplicon, const char* out_gaf,
                      int32_t n_threads);
int hs_gaf_from_labels(const char* gfa, const char* reads, const char* sam, int32_t amplicon, int32_t n_contigs,
                       const int64_t* win_off, const int32_t* win_start, const int32_t* win_end, const int64_t* label_off,
                       const int32_t* labels, const uint8_t* contig_has_snps, const char* out_gaf, int32_t n_threads);
int hs_gro_to_gaf_main(int argc, char** argv);

/* ------------------------------------------------------------------------------------------------
 * Next stage, the polisher's inputs (device work on the resident batch): for every merged interval of every contig and every
 * group of reads, the backbone piece and the pieces of the reads that the reference hands to its polisher.  Replaces the loop
 * of modify_GFA, create_new_contigs.cpp:358-521: the bounds of :371-375, the base-by-base CIGAR walk of :392-447 (on the
 * run-length ops, one wavefront per (interval, read)), the cut of the read or of its reverse complement (:453-459), the
 * clipped CIGAR (:460-462, convert_cigar2 of tools.cpp:61-80), the groups of :478-506 and toPolish of :517-519.  What
 * consensus_reads writes from them (tools.cpp:351-361) is what the tool below writes.  No consensus, no GFA.
 *
 * A bundle = one group of one interval; bundles come contig by contig, interval by interval, group label ascending (the
 * reference iterates an unordered_map).  A bundle exists only where the reference polishes: more than one cluster in the
 * interval, or polish_everything (:523).  Pieces of a bundle are in record order; piece k of a bundle is read<k> of
 * reads_<id>.fasta.  All arrays are host memory, released by hs_polish_result_destroy.
 * ---------------------------------------------------------------------------------------------- */
#define HS_POLISH_START_BEYOND_SEQ 2   /* piece_flags: posOnReadStart lies beyond the read (the reference's substr throws, :459): empty piece */
typedef struct hs_polish_result {
    int64_t n_bundles, n_pieces, n_dropped;
    /* per bundle */
    int32_t *bundle_contig, *bundle_interval /* index among the contig's merged intervals */, *bundle_start, *bundle_end, *bundle_group,
        *bundle_left_to_polish, *bundle_right_to_polish, *bundle_overhang_left, *bundle_overhang_right;   /* :371-375 */
    int64_t* backbone_off;      /* [n_bundles + 1] into backbone: toPolish (:517-519), text */
    uint8_t* backbone;
    int64_t* piece_off;         /* [n_bundles + 1]: the bundle's pieces */
    /* per piece */
    int32_t *piece_rec /* index of the record on its contig */, *piece_read_start, *piece_read_end /* posOnReadStart / posOnReadEnd */,
        *piece_sam_pos /* startPosition, :394-395 */, *piece_flags;
    int64_t* base_off;          /* [n_pieces + 1] into bases: clippedRead (:459), text */
    uint8_t* bases;
    int64_t* cig_off;           /* [n_pieces + 1] into cigar: clippedCIGAR (:460-462) as len << 4 | op words (none for an empty range) */
    uint32_t* cigar;
    int32_t* dropped;           /* [n_dropped][3]: contig, interval, record on the contig of the reads whose label became -2 (:444-447) */
    /* accounting (HIP events around the launches): the cursor table, k_polish_cut, k_polish_gather (reads + backbones), k_polish_cigar */
    double t_scan_ms, t_cut_ms, t_gather_ms, t_cigar_ms;
    int64_t n_tasks, n_rounds, cut_ops_read;   /* (interval, read) tasks; rounds of HS_POLISH_CHUNK_MB; CIGAR ops k_polish_cut loaded, in whole 64-op chunks */
} hs_polish_result;
/* windows + labels exactly as hs_gaf_from_labels takes them (all contigs of the batch); bundles of the contigs [c0, c1).
 * polish_everything: the contigs without partitions get the default interval of :249-251.  The output goes through device
 * scratch of HS_POLISH_CHUNK_MB (default 1024) megabytes: a larger call runs in several rounds over contig sub-ranges. */
int hs_polish_inputs(hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end,
                     const int64_t* label_off, const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything,
                     hs_polish_result** out);
/* the same from the four files HS_create_new_contigs reads (main, :1586-1595), written as text: per bundle a line
 * "BUNDLE <contig> <interval start> <interval end> <group> <leftToPolish> <rightToPolish> <overhangLeft> <overhangRight> <reads>"
 * (tab-separated), then ">seq" and toPolish, then per non-empty piece ">read<k> <startPosition> <CIGAR>" and the piece
 * (tools.cpp:351-361).  With HS_CONSENSUS=1 in the environment every bundle ends in ">consensus <trim_start> <trim_end>" and its
 * consensus (hs_polish_consensus below, the default parameters).  With HS_HAPLOTYPES=1 the FASTA of
 * hs_polish_haplotypes_from_files (below, the default parameters) is written in place of this text; where both are set,
 * HS_HAPLOTYPES wins. */
int hs_polish_inputs_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything,
                                const char* out_path, int32_t n_threads);
void hs_polish_result_destroy(hs_polish_result* r);
/* argv = <gfa> <reads> <sam> <gro> <polish_everything:0|1> <out> [threads] */
int hs_polish_inputs_main(int argc, char** argv);

/* ------------------------------------------------------------------------------------------------
 * The consensus of every bundle (device work): a vote per backbone column and per insertion slot over the bundle's pieces, what
 * the reference gets from minimap2 + racon (tools.cpp:317-...).  The rule is OURS, not racon's; it is stated once, in
 * csrc/hs_consensus_host.h, and the device is held to its host half by integer equality.
 *   walk of a piece: t = piece_sam_pos - 1, q = 0; M votes P[q] at column t, D votes deletion at t, I consumes read bases, any other
 *     op does nothing; votes at t >= L are dropped.  Skipped (n_skipped): an empty piece, HS_POLISH_START_BEYOND_SEQ, sum(M + I) !=
 *     its bases, piece_sam_pos - 1 >= L.
 *   column: fewer than min_cov covering pieces keep the byte B[t] (n_low); else the largest of A C G T deletion, B[t] on a tie it
 *     takes part in, else the first.  A winning deletion emits nothing (n_del), another base than B[t] is a substitution (n_sub).
 *   slot t (between t - 1 and t): span = pieces covering both, nins = those with an insertion there; wins iff span >= min_cov and
 *     2 nins > span.  Length = the most frequent (capped at max_ins) among the voters, the smaller on a tie; base j = the most
 *     frequent at offset j over voters longer than j, A < C < G < T on a tie (n_ins_bases).
 *   trim_start, trim_end: where the backbone columns min(overhang_left, L) and L - min(overhang_right, L) begin in the consensus
 *     (a column begins in front of its slot's insertion): cons[trim_start, trim_end) is the bundle without its overhangs, exactly --
 *     no alignment as in hs_trim_polished, and nothing to reattach.
 * min_cov 3 and max_ins 32 (allowed 1..64) are PLACEHOLDERS of the interface: nobody has tuned them.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_consensus_params { int32_t min_cov, max_ins; } hs_consensus_params;
hs_consensus_params hs_consensus_default_params(void);
typedef struct hs_consensus_result {
    int64_t n_bundles;
    int64_t* cons_off;          /* [n_bundles + 1] into cons: the consensus of every bundle, text (a bundle without pieces: its backbone) */
    uint8_t* cons;
    int32_t *trim_start, *trim_end, *n_sub, *n_del, *n_ins_bases, *n_low /* columns kept for low coverage */, *n_skipped /* pieces */;
    /* accounting (HIP events around the launches; 0 on the host half): rows, columns, insertion tables, scan + emit */
    double t_rows_ms, t_columns_ms, t_ins_ms, t_emit_ms;
    int64_t n_rounds /* of HS_CONSENSUS_CHUNK_MB */, n_ins_records /* insertions that voted */, n_ins_slots /* slots that won */;
} hs_consensus_result;
/* The arrays are those of a hs_polish_result, in host memory; they go up round by round, whole bundles within HS_CONSENSUS_CHUNK_MB
 * (default 1024) megabytes of row bytes (one per piece and covered column).  A single bundle above that is refused and named. */
int hs_polish_consensus(const hs_polish_result* in, const hs_consensus_params* params /* NULL: the defaults */, hs_consensus_result** out);
int hs_polish_consensus_arrays(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left,
                               const int32_t* overhang_right, const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags,
                               const int64_t* base_off, const uint8_t* bases, const int64_t* cig_off, const uint32_t* cigar,
                               const hs_consensus_params* params, hs_consensus_result** out);
/* the host half of the rule behind the same signature (no device needed): what the device is tested against.  The bundles are
 * strided over the host's threads, or over HS_CONSENSUS_HOST_THREADS of them. */
int hs_polish_consensus_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left,
                             const int32_t* overhang_right, const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags,
                             const int64_t* base_off, const uint8_t* bases, const int64_t* cig_off, const uint32_t* cigar,
                             const hs_consensus_params* params, hs_consensus_result** out);
void hs_consensus_result_destroy(hs_consensus_result* r);

/* ------------------------------------------------------------------------------------------------
 * From labels to haplotype sequences in one call (device work): the rounds of hs_polish_inputs with the consensus as their sink.  The
 * pieces, their clipped CIGARs and the backbones stay in device memory; the plan of every piece (hs::cons_piece_plan: skipped?,
 * covered columns, voting insertions) is computed there (k_cons_plan), and the rounds end in the kernels of hs_polish_consensus.
 * Host waits of a call: one for the cut table, one per resident round (of HS_POLISH_CHUNK_MB) for the plan's sizes, two per
 * consensus sub-round (whole bundles within HS_CONSENSUS_CHUNK_MB of row bytes) -- and one more on the first polishing call on a
 * batch, which fetches the records' strand, op ranges and reads once.  No new contigs, no GFA, no .gaf.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_haplotypes_result {
    hs_polish_result* inputs;        /* every bundle_* / piece_* / *_off / dropped array of hs_polish_inputs for the same call;
                                        backbone, bases and cigar are NULL: they never came down */
    hs_consensus_result* consensus;  /* as hs_polish_consensus of those inputs (n_rounds: the sub-rounds) */
    int64_t n_rounds, n_sub_rounds, bytes_down, bytes_up;   /* resident rounds, consensus sub-rounds, what the call moved */
    double t_plan_ms;                /* k_cons_plan + layout, HIP events */
} hs_haplotypes_result;
/* the arguments of hs_polish_inputs, then the consensus parameters (NULL: the defaults).  A bundle above HS_CONSENSUS_CHUNK_MB and a
 * CIGAR of more than 2^31 - 1 bases (M and D lengths plus M and I lengths: an M op counts twice) are refused with the messages of
 * hs_polish_consensus; a CIGAR of exactly 2^31 - 1 is accepted.  Both sides of that limit are tested (tests/haplotype_cases.py). */
int hs_polish_haplotypes(hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end,
                         const int64_t* label_off, const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything,
                         const hs_consensus_params* params, hs_haplotypes_result** out);
/* the same from the four files of hs_polish_inputs_from_files, written as FASTA (the format is ours): one record per bundle, in bundle
 * order; header ">" <contig name> "_" <bundle_start> "_" <bundle_end> "_" <bundle_group>; body the bundle's consensus
 * [trim_start, trim_end) on one line (an empty line where nothing is left). */
int hs_polish_haplotypes_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything,
                                    const hs_consensus_params* params, const char* out_fasta, int32_t n_threads);
void hs_haplotypes_result_destroy(hs_haplotypes_result* r);
/* test tap: the arrays of hs_polish_consensus_arrays, uploaded whole, but planned by k_cons_plan and laid out by the scans, as the
 * resident route plans them; plan_out [4 * n_pieces] (may be NULL) = skipped, long_cigar, n_cols, n_ins of every piece as the device
 * found them.  n_rounds of the result: the sub-rounds. */
int hs_polish_consensus_planned_tap(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left,
                                    const int32_t* overhang_right, const int64_t* piece_off, const int32_t* piece_sam_pos,
                                    const int32_t* piece_flags, const int64_t* base_off, const uint8_t* bases, const int64_t* cig_off,
                                    const uint32_t* cigar, const hs_consensus_params* params, int32_t* plan_out, hs_consensus_result** out);

/* ------------------------------------------------------------------------------------------------
 * Polishing passes (device work): what the reference gets from its second minimap2 run in front of racon (tools.cpp:317-...: the reads
 * are mapped to the contig to polish once more before the consensus).  hs_polish_haplotypes votes once, on the CIGARs the reads were given
 * against the CONTIG; where a haplotype has an indel inside a repeat every read's aligner may place the gap in another slot and no slot
 * wins.  A pass p >= 2 cuts every piece's window out of the consensus pass p - 1 made, aligns the piece to it (A1: edlibAlign NW, PATH,
 * k = -1), turns the moves into CIGAR words (the k_m2c_* kernels) and votes again with that consensus as the backbone.  The rule is
 * OURS; it is stated once, in csrc/hs_refine_host.h.  Everything between the passes stays in device memory: per pass and
 * consensus sub-round 16 bytes a piece come down (the windows: A1's launcher takes host offsets) and the bundles' offsets and counters;
 * only the last pass's text does.  n_passes passes run, there is no early stop.  n_passes = 1 is hs_polish_haplotypes, untouched.
 * Limits: a piece of more than 2^20 bases has no path (n_unaligned) and is skipped by the next pass; an A1 chunk (HS_REALIGN_CHUNK_MB)
 * holds at most 2^31 - 256 pairs and 2^31 - 1 move bytes.
 * ---------------------------------------------------------------------------------------------- */
#define HS_REFINE_MAX_PASSES 8
/* one pass on the host and what the next needs of it (no device): the consensus of hs_polish_consensus_host; per bundle b and column t in
 * [0, L] at col_off[b] + t: col_begin, where column t begins in the bundle's consensus (in front of its slot's insertion; column L: its
 * end), and col_ins, the inserted bases in front of column t; per piece its window [win_start, win_end) in its bundle's consensus
 * (-1 / -1: no window -- a skipped piece, or one that covers no column). */
typedef struct hs_refine_plan {
    hs_consensus_result* consensus;
    int64_t n_bundles, n_pieces;
    int64_t* col_off;           /* [n_bundles + 1] */
    int32_t *col_begin, *col_ins;
    int64_t *win_start, *win_end;
} hs_refine_plan;
int hs_polish_refine_plan_host(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left,
                               const int32_t* overhang_right, const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags,
                               const int64_t* base_off, const uint8_t* bases, const int64_t* cig_off, const uint32_t* cigar,
                               const hs_consensus_params* params, hs_refine_plan** out);
void hs_refine_plan_destroy(hs_refine_plan* r);
typedef struct hs_refined_result {
    hs_haplotypes_result* last;   /* consensus: the last pass's; inputs as hs_polish_haplotypes (NULL from hs_polish_refine_arrays) */
    int32_t n_passes, pad;
    /* per pass (index p - 1), summed over the bundles, each against that pass's backbone: the convergence figures */
    int64_t n_sub[HS_REFINE_MAX_PASSES], n_del[HS_REFINE_MAX_PASSES], n_ins_bases[HS_REFINE_MAX_PASSES], n_low[HS_REFINE_MAX_PASSES], n_skipped[HS_REFINE_MAX_PASSES];
    /* per pass from 2 on ([0] is 0): aligned pairs, pairs without a path, the sum of their edit distances, moves, CIGAR words */
    int64_t n_pairs[HS_REFINE_MAX_PASSES], n_unaligned[HS_REFINE_MAX_PASSES], sum_dist[HS_REFINE_MAX_PASSES], move_bytes[HS_REFINE_MAX_PASSES], cigar_words[HS_REFINE_MAX_PASSES];
    /* per pass: windows + gather (HIP events), A1 (wall, it synchronises), moves -> words (wall), the plan and the consensus (HIP events) */
    double t_windows_ms[HS_REFINE_MAX_PASSES], t_align_ms[HS_REFINE_MAX_PASSES], t_cigar_ms[HS_REFINE_MAX_PASSES], t_plan_ms[HS_REFINE_MAX_PASSES], t_consensus_ms[HS_REFINE_MAX_PASSES];
    int64_t n_waits[HS_REFINE_MAX_PASSES];   /* host waits of the pass, over all rounds (pass 1: those of the one-pass call) */
} hs_refined_result;
/* the arguments of hs_polish_haplotypes, then the number of passes: below 1 or above HS_REFINE_MAX_PASSES is HS_EINVAL and named */
int hs_polish_haplotypes_refined(hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end,
                                 const int64_t* label_off, const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything,
                                 const hs_consensus_params* params, int32_t n_passes, hs_refined_result** out);
/* the arrays of hs_polish_consensus_arrays, uploaded whole, then the resident route with passes (as hs_polish_consensus_planned_tap for one) */
int hs_polish_refine_arrays(int64_t n_bundles, const int64_t* backbone_off, const uint8_t* backbone, const int32_t* overhang_left,
                            const int32_t* overhang_right, const int64_t* piece_off, const int32_t* piece_sam_pos, const int32_t* piece_flags,
                            const int64_t* base_off, const uint8_t* bases, const int64_t* cig_off, const uint32_t* cigar,
                            const hs_consensus_params* params, int32_t n_passes, hs_refined_result** out);
/* hs_polish_haplotypes_from_files with passes (HS_POLISH_PASSES of bin/hs_polish_inputs) */
int hs_polish_haplotypes_refined_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything,
                                            const hs_consensus_params* params, int32_t n_passes, const char* out_fasta, int32_t n_threads);
void hs_refined_result_destroy(hs_refined_result* r);

/* ------------------------------------------------------------------------------------------------
 * Upstream feeders of stage 3 that are plain text transforms (host code): the 300 kb cutter the orchestrator runs before the
 * reads are aligned (src/cut_gfa.py:33-66, hairsplitter.py:583) and the GFA -> FASTA converter (src/gfa2fa.cpp).
 * hs_cut_gfa_main: argv of cut_gfa.py (--assembly/-a, --length/-l, --output/-o); hs_gfa2fa_main: argv[1] = gfa, FASTA on
 * standard output. Byte-identical to the reference's outputs (tests/golden/gfa_tools).
 * ---------------------------------------------------------------------------------------------- */
int hs_cut_gfa(const char* gfa_in, int64_t length, const char* gfa_out);
int hs_gfa_to_fasta(const char* gfa_in, const char* fasta_out /* NULL or "-": standard output */);
int hs_cut_gfa_main(int argc, char** argv);
int hs_gfa2fa_main(int argc, char** argv);

/* ------------------------------------------------------------------------------------------------
 * The step in front of the intervals: which contig window every read came from, on the device. Minimizer seeds
 * against a resident index of the contigs and a vote over diagonal bins; no chaining and no base-level alignment -- A1 places the
 * read inside the window (hs_realign_intervals). The reference has no counterpart (it shells out to minimap2); the rule is this
 * library's own, stated once in csrc/hs_map_host.h for host and device. hs_map_reads gives at most one interval per read (the primary);
 * hs_map_reads_split below adds the read's other parts as further intervals.
 * The defaults are minimap2's ONT k and w plus placeholders; they are not tuned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hs_map_params {
    int32_t k;             /* 5..16: bases of a k-mer (16: all 32 bits of the word in use); default 15 */
    int32_t w;             /* 1..32: k-mers of a minimizer window; default 10 */
    int32_t max_occ;       /* >= 1: a read minimizer whose hash has more index entries than this is not looked up; default 64 */
    int32_t band_log2;     /* 0..30: a diagonal bin is 2^band_log2 bases wide; default 9 */
    int32_t min_votes;     /* >= 1: hits in the best two adjacent bins for the read to count as mapped; default 3 */
    int32_t extend;        /* 0 | 1: stretch the seeds' interval to the whole read, clipped at the contig's ends; default 1 */
    int32_t bucket_bits;   /* 0..26: the index has 2^bucket_bits buckets (low bits of the hash); -1 (default): from the number of entries */
} hs_map_params;
hs_map_params hs_map_params_default(void);
typedef struct hs_map_index hs_map_index;
typedef struct hs_map_result {
    int32_t n_reads;
    /* per read; an unmapped read has contig -1 and zeros in the five fields behind it */
    int32_t* contig;
    uint8_t* strand;       /* 1 forward, 0 reverse, as hs_realign_intervals takes it */
    int32_t *qstart, *qend, *tstart, *tend;   /* half-open, 0-based; q on the read as given */
    int32_t *votes, *second;   /* score of the best candidate and of the best one elsewhere (0: none) */
    int32_t *n_minimizers, *n_skipped;   /* the read's minimizers; those not looked up (max_occ) */
    int64_t* n_hits;
    /* per call */
    int64_t n_wide;        /* reads with more hits than the LDS route holds, voted in global scratch */
    int64_t total_minimizers, total_hits;
    double t_minimizers_ms, t_hits_ms, t_vote_ms;   /* HIP events around the three groups of launches */
} hs_map_result;
/* codes 0..3, one per byte; contig c = h_contig_seq[h_contig_off[c] .. h_contig_off[c + 1]). params NULL: the defaults. The index stays
 * on the device until it is destroyed and serves any number of calls. */
int hs_map_index_create(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const hs_map_params* params, hs_map_index** index);
void hs_map_index_destroy(hs_map_index* index);
/* the index as the device holds it, for inspection: n_entries and bucket_bits; with non-NULL arrays also bucket_off [2^bucket_bits + 1] and the
 * entries' hash, contig and t << 1 | strand bit [n_entries]. The order inside a bucket is not defined. */
int hs_map_index_download(const hs_map_index* index, int64_t* n_entries, int32_t* bucket_bits, int64_t* bucket_off, uint32_t* e_hash, int32_t* e_contig, uint32_t* e_ts);
int hs_map_reads(const hs_map_index* index, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads, hs_map_result** result);
void hs_map_result_destroy(hs_map_result* result);
/* hits of a read that the vote sorts in LDS; a read with more goes through global scratch */
int32_t hs_map_lds_capacity(void);
/* hs_map_reads, then hs_realign_intervals on the mapped reads (interval i = the i-th mapped read, ascending): the resident batch, the records
 * and the map result. records / result may be NULL. pad as hs_realign_intervals takes it. */
int hs_map_to_batch(const hs_map_index* index, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq,
                    const int64_t* h_read_off, int32_t n_reads, int32_t pad, hs_cv_batch** batch, hs_realign_records** records, hs_map_result** result);
/* PAF lines of the mapped reads: column 10 = votes, 11 = tend - tstart, 12 = 255, tags s1:i:votes s2:i:second. Names may be NULL (r<i>, c<i>).
 * *text is released with hs_free_host. */
int hs_map_text(const hs_map_result* result, const char* const* read_names, const int64_t* h_read_off, const char* const* contig_names,
                const int64_t* h_contig_off, int32_t n_contigs, char** text);
/* the same from a job's files: the assembly (GFA S lines, or FASTA) and the reads -> the PAF lines, written to out_paf. n_threads < 1: all cores
 * (for loading). hs_map_main: argv = <gfa|fasta> <reads> <out.paf> [threads], the tool bin/hs_map. HS_call_variants with HS_MAP=1 does not read its
 * alignment argument: it maps the reads this way into <tmpDir>/hs_mapped.paf and takes that file the way HS_REALIGN=1 takes a PAF. */
int hs_map_files(const char* gfa, const char* reads, const char* out_paf, int32_t n_threads, const hs_map_params* params);
int hs_map_main(int argc, char** argv);

/* Split mappings: a read's parts on other contigs -- or elsewhere on the same one -- as further intervals, what a mapper's
 * supplementary lines give. Opt-in: up to max_segments intervals per read over disjoint stretches of it, found by repeating the vote over the
 * hits that overlap no stretch already taken (rule: csrc/hs_map_host.h, "split mappings"). A read with one segment has hs_map_reads' record.
 * No merging of collinear segments, no secondary placements of one stretch, no MAPQ. The four defaults are placeholders; they are not tuned. */
typedef struct hs_map_split_params {
    int32_t max_segments;  /* 1..8: most intervals of a read; default 4 */
    int32_t min_votes;     /* >= 1: hits a segment of a later round needs (round 0: hs_map_params.min_votes); default 3 */
    int32_t min_span;      /* >= 0: read bases the seeds of a later round's segment must span; default 100 */
    int32_t max_gap;       /* >= 0: two neighbouring segments further apart on the read than this are not extended towards each other; default 200 */
} hs_map_split_params;
hs_map_split_params hs_map_split_params_default(void);
typedef struct hs_map_segments {
    int32_t n_reads;
    int64_t n_segments;
    int64_t* seg_off;      /* [n_reads + 1]: read r has the segments seg_off[r] .. seg_off[r + 1], ascending by their start on the read */
    /* per segment */
    int32_t *read, *contig;
    uint8_t* strand;
    int32_t *qstart, *qend, *tstart, *tend;
    int32_t *votes, *second;   /* the segment's hits; round 0's `second` as hs_map_result has it, 0 in later rounds */
    int32_t* round;        /* the round that found the segment: 0 = the read's primary */
    /* per read */
    int32_t *n_minimizers, *n_skipped;
    int64_t* n_hits;
    int32_t *read_votes, *read_second;   /* round 0's vote, also of a read without a segment (hs_map_result's votes and second) */
    /* per call */
    int64_t n_wide;
    int64_t total_minimizers, total_hits;
    double t_minimizers_ms, t_hits_ms, t_vote_ms;
} hs_map_segments;
/* split NULL: the defaults. Parameters out of range: HS_EINVAL. */
int hs_map_reads_split(const hs_map_index* index, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads, const hs_map_split_params* split,
                       hs_map_segments** segments);
void hs_map_segments_destroy(hs_map_segments* segments);
/* hs_map_reads_split, then hs_realign_intervals with interval i = segment i: the counterpart of hs_map_to_batch. records / segments may be NULL. */
int hs_map_split_to_batch(const hs_map_index* index, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq,
                          const int64_t* h_read_off, int32_t n_reads, int32_t pad, const hs_map_split_params* split, hs_cv_batch** batch, hs_realign_records** records,
                          hs_map_segments** segments);
/* one PAF line per segment in segment order: hs_map_text's columns and s1 / s2 tags, then sg:i:<round> ns:i:<segments of the read>. With
 * HS_MAP_SPLIT=<n> (2..8) in the environment hs_map_files (bin/hs_map, HS_MAP=1) writes these lines with max_segments = n; unset or 1: hs_map_text's (any other value too, with a line on stderr).
 * seg_off must ascend from 0 to n_segments: HS_EINVAL otherwise. */
int hs_map_segments_text(const hs_map_segments* segments, const char* const* read_names, const int64_t* h_read_off, const char* const* contig_names,
                         const int64_t* h_contig_off, int32_t n_contigs, char** text);

/* Anchored alignment (opt-in; rule: csrc/hs_map_host.h, "anchors"). The hits of a mapped read's best candidate are exact k-mer matches along
 * its diagonal. Their chain, thinned to supported members at least `spacing` read bases apart, gives cut points (q, t): q on the read AS IT
 * ALIGNS (the read's own coordinate on strand 1, the coordinate in its reverse complement on strand 0), t on the contig. An interval cut at its
 * anchors is aligned piece by piece -- head (start free on the contig), middles (global), tail (end free) -- and the pieces' moves are joined
 * into one record. Such an alignment is a cheapest one THROUGH THE ANCHORS, not edlib's HW optimum in the window: NM(anchored) >= NM(plain).
 * An unmapped read has no anchors; neither has a read with more hits than hs_map_lds_capacity() (n_wide counts those): it is aligned the
 * plain way. spacing >= 1; the default 256 was a placeholder and is now the fastest of one sweep on one job; it is NOT tuned beyond that. */
typedef struct hs_map_anchor_params { int32_t spacing; } hs_map_anchor_params;
hs_map_anchor_params hs_map_anchor_params_default(void);
typedef struct hs_map_anchors {
    int32_t n_reads;
    int64_t n_anchors;
    int64_t* anc_off;                         /* [n_reads+1] */
    int32_t *anc_q, *anc_t;                   /* [n_anchors] (room for one at least): ascending in both inside a read */
    int32_t *n_best, *n_chain, *n_supported;  /* [n_reads] hits of the best, members of their chain, supported members (0: no anchors) */
    double t_anchors_ms;                      /* HIP events around k_map_anchors, the scan and the compaction */
} hs_map_anchors;
/* hs_map_reads plus the anchors of every read. `result` is field for field hs_map_reads' result; params NULL: the defaults; spacing < 1:
 * HS_EINVAL. Three waits, as hs_map_reads: the anchors leave in the per-read block's shipment. */
int hs_map_reads_anchored(const hs_map_index* index, const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads, const hs_map_anchor_params* params,
                          hs_map_result** result, hs_map_anchors** anchors);
void hs_map_anchors_destroy(hs_map_anchors* anchors);
/* hs_realign_intervals with the anchors of every interval given: anc_off [n_intervals+1], anc_q (read as it aligns) / anc_t (contig). The
 * alignment of an interval is a cheapest one THROUGH ITS ANCHORS, not edlib's HW optimum; an interval without anchors gets hs_realign_intervals'
 * record. Anchors of interval i must ascend strictly in q and in t with a0 <= q <= a1 and tstart <= t <= tend ([a0, a1) = the interval's read
 * range as it aligns): HS_EINVAL otherwise, and hs_last_error() names the interval. The pieces of an interval stay in one round and count
 * towards its pair limit; an interval with a piece the aligner has no path for is dropped. records->n_pieces / t_join_ms say what was done. */
int hs_realign_intervals_anchored(const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs,
                                  const uint8_t* h_read_seq, const int64_t* h_read_off, int32_t n_reads,
                                  const int32_t* iv_read, const int32_t* iv_contig, const uint8_t* iv_strand,
                                  const int32_t* iv_qstart, const int32_t* iv_qend, const int32_t* iv_tstart, const int32_t* iv_tend,
                                  int32_t n_intervals, int32_t pad, const int64_t* anc_off, const int32_t* anc_q, const int32_t* anc_t,
                                  hs_realign_records** out, struct hs_cv_batch** batch /* may be NULL */);
/* hs_map_reads_anchored, then hs_realign_intervals_anchored on the mapped reads with their anchors: hs_map_to_batch's counterpart; the
 * alignments are cheapest ones through the anchors, not edlib's HW optima. records / result / anchors may be NULL. */
int hs_map_to_batch_anchored(const hs_map_index* index, const uint8_t* h_contig_seq, const int64_t* h_contig_off, int32_t n_contigs, const uint8_t* h_read_seq,
                             const int64_t* h_read_off, int32_t n_reads, int32_t pad, const hs_map_anchor_params* params, hs_cv_batch** batch,
                             hs_realign_records** records, hs_map_result** result, hs_map_anchors** anchors);

/* Test taps of the two device steps around A1 on the CIGAR-less route (hs_kernels_realign.hip), each through the launch the job itself makes; host
 * arrays in, host arrays out, nothing on the product path. Both check their tables on the host before any launch and refuse with HS_EINVAL and a
 * message: no table they accept can make a kernel read or write outside its buffers.
 *
 * hs_realign_cut_tap -- k_realign_cut. `seq` goes up as the job's sequences do (HS_SEQ_PAD zero bytes on either side); piece i of the output is
 * out[off[i], off[i + 1]): seq[src[i]], seq[src[i] + 1], ... or, where rev[i] is set, 3 - seq[src[i]], 3 - seq[src[i] - 1], ... as a byte. The
 * out_cap device bytes are set to the byte `fill` before the launch and all come back, so the bytes behind off[m] rounded up to 16 are guards.
 * Refused: m < 1, off that does not ascend strictly from 0, a piece that leaves [0, seq_len) at either end, out_cap below off[m] rounded up to 16. */
int hs_realign_cut_tap(const uint8_t* seq, int64_t seq_len, const int64_t* off /* [m + 1] */, const int64_t* src /* [m] */, const uint8_t* rev /* [m], may be NULL */,
                       int32_t m, int32_t fill, uint8_t* out, int64_t out_cap);
/* hs_anchor_join_tap -- k_anchor_join_plan and k_anchor_join on a piece table as hs_realign_intervals_anchored builds it per round: interval k has the
 * pieces [iv_piece[k], iv_piece[k + 1]) and the room [join_off[k], join_off[k + 1]) in the joined buffer; piece p is of kind pc_kind[p] (0 HW, 1 HEAD,
 * 2 MID, 3 TAIL, 4 INS), has room for pc_room[p] moves at ops + pc_ops[p] and its numbers at index pc_idx[p] of dist / start / end / len (INS: pc_idx is
 * the run's length, pc_ops is not used). The aligner's side is given: ops [ops_bytes] and the n_num numbers. joined_cap device bytes are set to `fill`
 * before the launches and all come back; pc_at [iv_piece[m]], out_len / out_dist / out_pos [m] as the plan leaves them.
 * Refused: m < 1; iv_piece that does not ascend strictly from 0; join_off that does not ascend from 0; a kind above 4; a pc_idx outside [0, n_num) (INS
 * excepted); a negative pc_room, or pc_ops + pc_room outside [0, ops_bytes] (INS excepted); an interval whose room is below the sum of its pieces' rooms
 * or above 2^31 - 1; joined_cap below join_off[m] rounded up to 16. */
int hs_anchor_join_tap(int32_t m, const int32_t* iv_piece /* [m + 1] */, const int32_t* iv_base /* [m] */, const int64_t* join_off /* [m + 1] */,
                       const uint8_t* pc_kind, const int32_t* pc_idx, const int32_t* pc_room, const int64_t* pc_ops /* [iv_piece[m]] each */,
                       const uint8_t* ops, int64_t ops_bytes, const int32_t* dist, const int32_t* start, const int32_t* end, const int32_t* len, int32_t n_num,
                       int32_t fill, int32_t* pc_at, int32_t* out_len, int32_t* out_dist, int32_t* out_pos, uint8_t* joined, int64_t joined_cap);

#ifdef __cplusplus
}
#endif
#endif /* HAIRSPLITTER_HIP_H */
