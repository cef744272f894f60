// hs_capi_kernels.inc -- part of hs_capi.hip: the small C ABI (version, device, memory, events, kernel statistics) and the
// kernel-level entry points (one launch or a short family each: K0/K1 pileup, K2 column statistics, gather, top-3, K4, K5a/K5, Chinese
// Whispers, A1), as include/hairsplitter_hip.h declares them.
extern "C" {

const char* hs_version(void) { return "hairsplitter_amd 0.3 (gfx950)"; }
const char* hs_kernel_name(int k) {
    static const char* names[HS_NKERNELS] = {"k_cigar_scan", "k_pileup_runs", "k_column_stats_tiled", "k_columns_compact", "k_gather_tiles", "k_column_top3_exact",
                                             "k_candidates_scan", "k_pack_flagged", "k_partition_transpose", "k_column_partition_lanes", "k_column_partition_test",
                                             "k_snp_flags", "k_window_masks", "k_snp_planes", "k_simdiff", "k_read_graph_rows", "k_read_graph_fill", "k_cw_visit_lists",
                                             "k_cw_seed_sets", "k_cw_seeded_lanes", "k_cw_seeded_rows", "k_window_tail", "k_cw_local", "k_loop_a", "other", "k_cand_bits", "k_ship", "k_column_partition_grouped"};
    return k >= 0 && k < HS_NKERNELS ? names[k] : "?";
}
void hs_kernel_stats_reset(void) { KernelTable& t = kernel_table(); std::lock_guard<std::mutex> g(t.mu); std::memset(&t.st, 0, sizeof t.st); }
void hs_kernel_stats_get(hs_kernel_stats* out) { if (!out) return; KernelTable& t = kernel_table(); std::lock_guard<std::mutex> g(t.mu); *out = t.st; }
const char* hs_last_error(void) { return hs::g_err.c_str(); }
// host waits for the device since the library was loaded (every one is a round trip of a contig group's chain); the wall time
// spent in them is only kept under HS_TIMING
void hs_kernel_stats_every(int32_t n) { g_timing_every.store(n < 1 ? 1 : n); g_timing_step.store(0); g_timing_on.store(true); }
void hs_host_wait_stats(int64_t* n_waits, double* ms_in_waits) { if (n_waits) *n_waits = g_waits.load(); if (ms_in_waits) *ms_in_waits = g_wait_us.load() / 1e3; }
int hs_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
static std::vector<int> device_list();
int hs_warmup(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
    // every device the stage calls will use (HS_DEVICES / all visible), side by side: context + code object of each
    std::vector<int> devs = device_list();
    std::sort(devs.begin(), devs.end());
    devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
    if (devs.empty()) devs.push_back(0);
    auto warm_one = [](int dev) {
        if (hipSetDevice(dev) != hipSuccess) return;
        void* p = nullptr;
        if (hipMalloc(&p, 256) != hipSuccess) return;
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, 0, (uint4*)p, 0ll, 0u);   // loads the code object
        (void)hipDeviceSynchronize();
        (void)hipFree(p);
    };
    std::vector<std::thread> th;
    for (size_t i = 1; i < devs.size(); ++i) th.emplace_back(warm_one, devs[i]);
    warm_one(devs[0]);
    for (auto& t : th) t.join();
    (void)hipSetDevice(devs[0]);
    return n;
}
int hs_set_device(int device) { HS_HIP(hipSetDevice(device)); set_wait_policy(); return HS_OK; }
int hs_device_synchronize(void) { HS_HIP(hipDeviceSynchronize()); return HS_OK; }
int hs_malloc(void** d_ptr, size_t bytes) { HS_HIP(hipMalloc(d_ptr, bytes ? bytes : 16)); return HS_OK; }
int hs_free(void* d_ptr) { HS_HIP(hipFree(d_ptr)); return HS_OK; }
int hs_memcpy_h2d(void* d, const void* h, size_t n) { if (n) HS_HIP(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); return HS_OK; }
int hs_memcpy_d2h(void* h, const void* d, size_t n) { if (n) HS_HIP(hipMemcpy(h, d, n, hipMemcpyDeviceToHost)); return HS_OK; }
int hs_memset(void* d, int v, size_t n) { if (n) HS_HIP(hipMemset(d, v, n)); return HS_OK; }
int hs_event_create(void** ev) { hipEvent_t e; HS_HIP(hipEventCreate(&e)); *ev = (void*)e; return HS_OK; }
int hs_event_destroy(void* ev) { HS_HIP(hipEventDestroy((hipEvent_t)ev)); return HS_OK; }
int hs_event_record(void* ev, void* stream) { HS_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return HS_OK; }
int hs_event_elapsed_ms(void* a, void* b, float* ms) {
    HS_HIP(hipEventSynchronize((hipEvent_t)b));
    HS_HIP(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return HS_OK;
}

// ---------------------------------------------------------------------------------------------------
// kernel-level entry points
// ---------------------------------------------------------------------------------------------------
static int cigar_scan_launch(const int64_t* d_contig_off, const int32_t* d_rec_contig, const int32_t* d_rec_pos, const int64_t* d_rec_cig_off,
                             const uint32_t* d_cigar, const int64_t* d_rec_chunk_off, int32_t n_rec, int32_t* d_chunk_scratch, int32_t* d_rec_stats,
                             void* stream) {
    if (n_rec <= 0) return HS_OK;
    hipLaunchKernelGGL(hsdev::k_cigar_scan, dim3((n_rec + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_contig_off, d_rec_contig,
                       d_rec_pos, d_rec_cig_off, d_cigar, d_rec_chunk_off, n_rec, d_chunk_scratch, d_rec_stats);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

// tasks of k_pileup_runs: (record, first chunk) for every HS_K1R_NCH 64-op chunks of K0's table
static void build_run_tasks(const int64_t* h_rec_chunk_off, int32_t n_rec, std::vector<int32_t>& task_rec, std::vector<int32_t>& task_chunk, std::vector<int32_t>* rec_task_off) {
    task_rec.clear(); task_chunk.clear();
    if (rec_task_off) rec_task_off->assign((size_t)n_rec + 1, 0);
    for (int32_t r = 0; r < n_rec; ++r) {
        const int64_t nc = h_rec_chunk_off[r + 1] - h_rec_chunk_off[r];
        for (int64_t k = 0; k < nc; k += HS_K1R_NCH) { task_rec.push_back(r); task_chunk.push_back((int32_t)k); }
        if (rec_task_off) (*rec_task_off)[(size_t)r + 1] = (int32_t)task_rec.size();
    }
}
// the task list as k_pileup_runs reads it: one 64-byte record per task (k_run_task_desc) from the (record, chunk) pairs and the batch's arrays
static int run_task_records(const int32_t* d_task_rec, const int32_t* d_task_chunk, int32_t n, const int64_t* d_contig_off, const int64_t* d_read_off,
                            const int32_t* d_rec_read, const int32_t* d_rec_contig, const int32_t* d_rec_pos, const uint8_t* d_rec_strand,
                            const int64_t* d_rec_cig_off, const int64_t* d_pile_off, const int64_t* d_rec_chunk_off, void* d_out, void* stream,
                            const uint32_t* d_cigar, uint32_t* d_ops_out /* [n * 64 * HS_K1R_NCH]: the tasks' ops (k_run_task_ops) */) {
    if (n <= 0) return HS_OK;
    hipLaunchKernelGGL(hsdev::k_run_task_desc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_task_rec, d_task_chunk, n, d_contig_off,
                       d_read_off, d_rec_read, d_rec_contig, d_rec_pos, d_rec_strand, d_rec_cig_off, d_pile_off, d_rec_chunk_off, (int)HS_K1R_NCH,
                       static_cast<hsdev::RunTask*>(d_out));
    {
        const long long total = (long long)n * 64 * HS_K1R_NCH;
        hipLaunchKernelGGL(hsdev::k_run_task_ops, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, static_cast<const hsdev::RunTask*>(d_out), n, d_cigar,
                           (int)(64 * HS_K1R_NCH), d_ops_out);
    }
    HS_HIP(hipGetLastError());
    return HS_OK;
}
#define HS_RUN_TASK_BYTES 64
#define HS_RUN_TASK_OPS_BYTES (64 * HS_K1R_NCH * 4)
#define HS_SEQ_PAD 64      /* readable bytes before and after the contig / read bases handed to k_pileup_runs */

// K1 (k_pileup_runs) over a task list of hsdev::RunTask records (run_task_records below; the sequences padded by HS_SEQ_PAD), then the few
// records it leaves out (K0 flagged them: a clip between aligned bases) per event. Record-indexed arrays are passed whole (tasks name
// records by their index in them); `r0 / nr`: the records of the launch (the flagged ones among them are walked by k_pileup_flagged_records).
static int pileup_launch(const uint8_t* d_contig_seq, const int64_t* d_contig_off, const uint8_t* d_read_seq,
                         const int64_t* d_read_off, const int32_t* d_rec_read, const int32_t* d_rec_contig,
                         const int32_t* d_rec_pos, const uint8_t* d_rec_strand, const int64_t* d_rec_cig_off,
                         const uint32_t* d_cigar, const int64_t* d_pile_off, const int64_t* d_rec_chunk_off,
                         int32_t* d_chunk_scratch, int32_t ev_per_task, uint8_t* d_pile, int32_t* d_rec_stats, int32_t r0, int32_t nr, void* stream,
                         const void* d_run_tasks, int32_t n_run, const uint32_t* d_run_ops) {
    if (n_run > 0)
        hipLaunchKernelGGL(hsdev::k_pileup_runs, dim3((n_run + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_contig_seq, d_read_seq, d_run_ops,
                           d_chunk_scratch, static_cast<const hsdev::RunTask*>(d_run_tasks), n_run, d_pile, d_rec_stats);
    if (nr > 0) {
        const int blocks = std::max(1, std::min(256, (nr + 255) / 256));
        hipLaunchKernelGGL(hsdev::k_pileup_flagged_records, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_contig_seq, d_contig_off,
                           d_read_seq, d_read_off, d_rec_read + r0, d_rec_contig + r0, d_rec_pos + r0, d_rec_strand + r0, d_rec_cig_off + r0, d_cigar,
                           d_pile_off + r0, d_rec_chunk_off + r0, d_chunk_scratch, nr, ev_per_task, d_pile, d_rec_stats + 4 * (size_t)r0);
    }
    HS_HIP(hipGetLastError());
    return HS_OK;
}

int hs_pileup(const uint8_t* d_contig_seq, const int64_t* d_contig_off, const uint8_t* d_read_seq,
              const int64_t* d_read_off, const int32_t* d_rec_read, const int32_t* d_rec_contig,
              const int32_t* d_rec_pos, const uint8_t* d_rec_strand, const int64_t* d_rec_cig_off,
              const uint32_t* d_cigar, const int64_t* d_pile_off, int32_t n_rec, const int64_t* d_rec_chunk_off,
              int32_t* d_chunk_scratch, const int32_t* d_task_rec, const int32_t* d_task_ev0, int32_t n_tasks,
              int32_t ev_per_task, uint8_t* d_pile, int32_t* d_rec_stats, void* stream) {
    if (int rc = require_device()) return rc;
    if (n_rec <= 0) return HS_OK;
    if (int rc = cigar_scan_launch(d_contig_off, d_rec_contig, d_rec_pos, d_rec_cig_off, d_cigar, d_rec_chunk_off, n_rec, d_chunk_scratch,
                                   d_rec_stats, stream)) return rc;
    (void)d_task_rec; (void)d_task_ev0; (void)n_tasks;      // (the event-range tasks of the forms of rounds 1-4: not read any more)
    // The run form reads up to HS_SEQ_PAD bytes beyond either end of the sequences and takes its own task list (pairs of op chunks):
    // this kernel-level entry -- the caller's arrays are what they are -- copies the sequences into padded scratch and derives the
    // tasks from the chunk table (the stage drivers keep both with the resident batch)
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> h_chunk_off((size_t)n_rec + 1), h_cig_off((size_t)n_rec + 1), h_tail(2);
    HS_HIP(hipMemcpyAsync(h_chunk_off.data(), d_rec_chunk_off, sizeof(int64_t) * ((size_t)n_rec + 1), hipMemcpyDeviceToHost, st));
    // sizes of the two sequence arrays: the contig / read of the highest index any record names is not known here; the offsets of the
    // LAST contig / read are found by reading the offset arrays up to the largest index among the records
    std::vector<int32_t> h_rc((size_t)n_rec), h_rr((size_t)n_rec);
    HS_HIP(hipMemcpyAsync(h_rc.data(), d_rec_contig, sizeof(int32_t) * (size_t)n_rec, hipMemcpyDeviceToHost, st));
    HS_HIP(hipMemcpyAsync(h_rr.data(), d_rec_read, sizeof(int32_t) * (size_t)n_rec, hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    int32_t cmax = 0, rmax = 0;
    for (int32_t r = 0; r < n_rec; ++r) { cmax = std::max(cmax, h_rc[(size_t)r]); rmax = std::max(rmax, h_rr[(size_t)r]); }
    int64_t c_end = 0, r_end = 0;
    HS_HIP(hipMemcpyAsync(&c_end, d_contig_off + cmax + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HS_HIP(hipMemcpyAsync(&r_end, d_read_off + rmax + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    std::vector<int32_t> tr, tc;
    build_run_tasks(h_chunk_off.data(), n_rec, tr, tc, nullptr);
    DBuf d_cs, d_rs, d_tr, d_tc, d_td, d_to;
    if (int rc = d_cs.alloc((size_t)c_end + 2 * HS_SEQ_PAD)) return rc;
    if (int rc = d_rs.alloc((size_t)r_end + 2 * HS_SEQ_PAD)) return rc;
    HS_HIP(hipMemsetAsync(d_cs.p, 0, HS_SEQ_PAD, st)); HS_HIP(hipMemsetAsync((char*)d_cs.p + HS_SEQ_PAD + c_end, 0, HS_SEQ_PAD, st));
    HS_HIP(hipMemsetAsync(d_rs.p, 0, HS_SEQ_PAD, st)); HS_HIP(hipMemsetAsync((char*)d_rs.p + HS_SEQ_PAD + r_end, 0, HS_SEQ_PAD, st));
    if (c_end) HS_HIP(hipMemcpyAsync((char*)d_cs.p + HS_SEQ_PAD, d_contig_seq, (size_t)c_end, hipMemcpyDeviceToDevice, st));
    if (r_end) HS_HIP(hipMemcpyAsync((char*)d_rs.p + HS_SEQ_PAD, d_read_seq, (size_t)r_end, hipMemcpyDeviceToDevice, st));
    if (int rc = d_tr.alloc(std::max<size_t>(1, tr.size()) * 4)) return rc;
    if (int rc = d_tc.alloc(std::max<size_t>(1, tc.size()) * 4)) return rc;
    if (!tr.empty()) { HS_HIP(hipMemcpyAsync(d_tr.p, tr.data(), tr.size() * 4, hipMemcpyHostToDevice, st)); HS_HIP(hipMemcpyAsync(d_tc.p, tc.data(), tc.size() * 4, hipMemcpyHostToDevice, st)); }
    if (int rc = d_td.alloc(std::max<size_t>(1, tr.size()) * HS_RUN_TASK_BYTES)) return rc;
    if (int rc = d_to.alloc(std::max<size_t>(1, tr.size()) * HS_RUN_TASK_OPS_BYTES)) return rc;
    if (int rc = run_task_records(d_tr.as<int32_t>(), d_tc.as<int32_t>(), (int32_t)tr.size(), d_contig_off, d_read_off, d_rec_read, d_rec_contig, d_rec_pos, d_rec_strand,
                                  d_rec_cig_off, d_pile_off, d_rec_chunk_off, d_td.p, stream, d_cigar, d_to.as<uint32_t>())) return rc;
    if (int rc = pileup_launch((const uint8_t*)d_cs.p + HS_SEQ_PAD, d_contig_off, (const uint8_t*)d_rs.p + HS_SEQ_PAD, d_read_off, d_rec_read, d_rec_contig, d_rec_pos, d_rec_strand,
                               d_rec_cig_off, d_cigar, d_pile_off, d_rec_chunk_off, d_chunk_scratch,
                               ev_per_task, d_pile, d_rec_stats, 0, n_rec, stream, d_td.p, (int32_t)tr.size(), d_to.as<uint32_t>())) return rc;
    HS_HIP(hipStreamSynchronize(st));      // (the scratch of this call goes back to the pool when it returns)
    return HS_OK;
}

#ifdef HS_K1R_PROFILE
int hs_debug_k1_profile(unsigned int* out, long long n_words) {      // (diagnostic build only) eight words per task
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hsdev::g_k1r_prof), (size_t)n_words * 4) != hipSuccess) return HS_EHIP;
    return HS_OK;
}
#endif
int hs_pileup_plan(const int64_t* h_rec_cig_off, const uint32_t* h_cigar, int32_t n_rec, int32_t ev_per_task,
                   int64_t* h_rec_chunk_off, int32_t* n_tasks, int32_t** h_task_rec, int32_t** h_task_ev0) {
    if (ev_per_task <= 0 || !h_rec_chunk_off || !n_tasks || !h_task_rec || !h_task_ev0) { set_error("hs_pileup_plan: bad arguments"); return HS_EINVAL; }
    std::vector<int32_t> tr, te;
    h_rec_chunk_off[0] = 0;
    std::vector<int64_t> ev_of((size_t)std::max(n_rec, 0));
    {   // events per record: one pass over all CIGAR ops, blocks of records on the host threads
        const int nb = std::max(1, std::min(n_rec / 256 + 1, 256));
        hs::hs_parallel_for(nb, host_threads(), [&](int b) {
            const int r0 = (int)((int64_t)n_rec * b / nb), r1 = (int)((int64_t)n_rec * (b + 1) / nb);
            for (int r = r0; r < r1; ++r) {
                int64_t ev = 0;
                for (int64_t o = h_rec_cig_off[r]; o < h_rec_cig_off[r + 1]; ++o) {
                    const uint32_t op = h_cigar[o] & 15u;
                    if (op == 0 || op == 1 || op == 2 || op == 7 || op == 8) ev += h_cigar[o] >> 4;
                }
                ev_of[(size_t)r] = ev;
            }
        });
    }
    for (int r = 0; r < n_rec; ++r) {
        const int64_t ev = ev_of[(size_t)r];
        if (ev > 0x7fffffff) { set_error("alignment with more than 2^31 events"); return HS_EINVAL; }
        h_rec_chunk_off[r + 1] = h_rec_chunk_off[r] + (h_rec_cig_off[r + 1] - h_rec_cig_off[r] + 63) / 64;
        for (int64_t e = 0; e < ev; e += ev_per_task) { tr.push_back(r); te.push_back((int32_t)e); }
    }
    *n_tasks = (int32_t)tr.size();
    *h_task_rec = (int32_t*)std::malloc(std::max<size_t>(1, tr.size()) * sizeof(int32_t));
    *h_task_ev0 = (int32_t*)std::malloc(std::max<size_t>(1, te.size()) * sizeof(int32_t));
    if (!tr.empty()) { std::memcpy(*h_task_rec, tr.data(), tr.size() * sizeof(int32_t)); std::memcpy(*h_task_ev0, te.data(), te.size() * sizeof(int32_t)); }
    return HS_OK;
}
void hs_free_host(void* p) { std::free(p); }

// exclusive scan of n ints into n + 1 offsets (see hs_kernels_graph.hip); the tile scratch (room for 2 * scan_tiles(n) words) must outlive
// the launches -- the caller's own, or a DBuf sized here
static int scan_tiles(int64_t n) { return (int)((n + HS_SCAN_TILE - 1) / HS_SCAN_TILE); }
static int exclusive_scan_launch(const int32_t* d_in, int n, int64_t* d_out, long long* tile_sum, hipStream_t stream) {
    const int n_tiles = scan_tiles(n);
    if (n_tiles == 0) { HS_HIP(hipMemsetAsync(d_out, 0, sizeof(int64_t), stream)); return HS_OK; }
    long long* tile_off = tile_sum + n_tiles;
    hipLaunchKernelGGL(hsdev::k_scan_tile_sums, dim3((unsigned)n_tiles), dim3(256), 0, stream, d_in, n, tile_sum);
    hipLaunchKernelGGL(hsdev::k_scan_tile_offsets, dim3(1), dim3(1024), 0, stream, tile_sum, n_tiles, tile_off, d_out + n);
    hipLaunchKernelGGL(hsdev::k_scan_apply, dim3((unsigned)n_tiles), dim3(256), 0, stream, d_in, n, tile_off, d_out);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
static int exclusive_scan_launch(const int32_t* d_in, int n, int64_t* d_out, DBuf& scratch, hipStream_t stream) {
    if (n > 0) { if (int rc = scratch.alloc((size_t)scan_tiles(n) * 16)) return rc; }
    return exclusive_scan_launch(d_in, n, d_out, scratch.as<long long>(), stream);
}

// K2's selection list: the kernels fill 256 scratch slots + one count per tile; scan + compact give the sorted list and its
// length (see column_stats_tail in hs_kernels.hip)
struct SelectionScratch {
    DBuf tile_cnt, tile_base, gpos, depth, scan_scratch;
    int64_t n_tiles = 0;
    int prepare(int64_t total_len) {
        n_tiles = (total_len + 255) / 256;
        if (int rc = tile_cnt.alloc((size_t)n_tiles * 4)) return rc;
        if (int rc = tile_base.alloc(((size_t)n_tiles + 1) * 8)) return rc;
        if (int rc = gpos.alloc((size_t)n_tiles * 256 * 8)) return rc;
        return depth.alloc((size_t)n_tiles * 256 * 4);
    }
    int finish(int32_t* d_sel_count, int64_t* d_sel_gpos, int32_t* d_sel_depth, int32_t sel_cap, hipStream_t stream) {
        if (n_tiles > 0x7fffffff) { set_error("too many tiles"); return HS_EINVAL; }
        if (int rc = exclusive_scan_launch(tile_cnt.as<int32_t>(), (int)n_tiles, tile_base.as<int64_t>(), scan_scratch, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_selection_compact, dim3((unsigned)n_tiles), dim3(256), 0, stream, tile_cnt.as<int32_t>(), tile_base.as<int64_t>(),
                           gpos.as<int64_t>(), depth.as<int32_t>(), n_tiles, d_sel_count, d_sel_gpos, d_sel_depth, sel_cap);
        HS_HIP(hipGetLastError());
        return HS_OK;
    }
};

namespace {
// the tile plan of include/hairsplitter_hip.h from host vectors
void build_tile_plan(const int64_t* contig_off, int n_contigs, const int32_t* contig_rec_off, const int32_t* rec_pos, const int32_t* rec_qend,
                     const int64_t* pile_off, std::vector<int64_t>& tile_off, std::vector<hs_tile_entry>& ent, std::vector<int32_t>& rec) {
    const int64_t total = n_contigs > 0 ? contig_off[n_contigs] : 0;
    const int64_t n_tiles = (total + 255) / 256;
    tile_off.assign((size_t)n_tiles + 1, 0);
    // Tiles are 256 positions of the concatenated contigs: only a contig's first and last tile can hold records of another contig. The
    // tiles in between are the contig's own -- counted and filled on the host threads, a contig per task --, the two shared ones are done
    // by one thread in record order (inside every tile the records ascend: the gather kernels rely on it).
    const int nt = host_threads();
    auto each_own = [&](int c, auto&& f) {      // f(record, tile, gs, ge) for the contig's records over its own tiles, records ascending
        const int64_t tf = contig_off[c] >> 8, tl = (contig_off[c + 1] - 1) >> 8;
        for (int r = contig_rec_off[c]; r < contig_rec_off[c + 1]; ++r) {
            if (rec_qend[r] <= rec_pos[r]) continue;
            const int64_t gs = contig_off[c] + rec_pos[r], ge = contig_off[c] + rec_qend[r];
            const int64_t ta = std::max(gs >> 8, tf + 1), tb = std::min((ge - 1) >> 8, tl - 1);
            for (int64_t t = ta; t <= tb; ++t) f(r, t, gs, ge);
        }
    };
    auto each_shared = [&](auto&& f) {          // the same over every contig's first and last tile, contigs and records ascending
        for (int c = 0; c < n_contigs; ++c) {
            if (contig_off[c + 1] <= contig_off[c]) continue;
            const int64_t tf = contig_off[c] >> 8, tl = (contig_off[c + 1] - 1) >> 8;
            for (int r = contig_rec_off[c]; r < contig_rec_off[c + 1]; ++r) {
                if (rec_qend[r] <= rec_pos[r]) continue;
                const int64_t gs = contig_off[c] + rec_pos[r], ge = contig_off[c] + rec_qend[r];
                const int64_t ta = gs >> 8, tb = (ge - 1) >> 8;
                if (ta <= tf && tf <= tb) f(r, tf, gs, ge);
                if (tl != tf && ta <= tl && tl <= tb) f(r, tl, gs, ge);
            }
        }
    };
    hs::hs_parallel_for(n_contigs, nt, [&](int c) { each_own(c, [&](int, int64_t t, int64_t, int64_t) { tile_off[(size_t)t + 1]++; }); });
    each_shared([&](int, int64_t t, int64_t, int64_t) { tile_off[(size_t)t + 1]++; });
    for (int64_t t = 0; t < n_tiles; ++t) tile_off[(size_t)t + 1] += tile_off[(size_t)t];
    ent.resize((size_t)tile_off[(size_t)n_tiles]); rec.resize(ent.size());
    std::vector<int64_t> fill(tile_off.begin(), tile_off.end() - 1);
    auto put = [&](int r, int64_t t, int64_t gs, int64_t ge) {
        const int64_t k = fill[(size_t)t]++;
        const int32_t first = (int32_t)(gs - t * 256);
        ent[(size_t)k] = hs_tile_entry{first, (int32_t)(ge - gs), pile_off[r] - first};
        rec[(size_t)k] = r;
    };
    each_shared(put);
    hs::hs_parallel_for(n_contigs, nt, [&](int c) { each_own(c, put); });
}
}  // namespace

int hs_tile_plan(const int64_t* h_contig_off, int32_t n_contigs, const int32_t* h_contig_rec_off, const int32_t* h_rec_pos,
                 const int32_t* h_rec_qend, const int64_t* h_pile_off, int64_t** tile_off, hs_tile_entry** tile_ent, int32_t** tile_rec,
                 int64_t* n_tiles) {
    if (!tile_off || !tile_ent || !tile_rec || !n_tiles || n_contigs < 0) { set_error("hs_tile_plan: bad arguments"); return HS_EINVAL; }
    std::vector<int64_t> to; std::vector<hs_tile_entry> en; std::vector<int32_t> rc;
    build_tile_plan(h_contig_off, n_contigs, h_contig_rec_off, h_rec_pos, h_rec_qend, h_pile_off, to, en, rc);
    *n_tiles = (int64_t)to.size() - 1;
    *tile_off = (int64_t*)std::malloc(to.size() * sizeof(int64_t));
    *tile_ent = (hs_tile_entry*)std::malloc((en.size() + 1) * sizeof(hs_tile_entry));
    *tile_rec = (int32_t*)std::malloc((rc.size() + 1) * sizeof(int32_t));
    if (!*tile_off || !*tile_ent || !*tile_rec) { set_error("hs_tile_plan: out of memory"); return HS_EINVAL; }
    std::memcpy(*tile_off, to.data(), to.size() * sizeof(int64_t));
    if (!en.empty()) { std::memcpy(*tile_ent, en.data(), en.size() * sizeof(hs_tile_entry)); std::memcpy(*tile_rec, rc.data(), rc.size() * sizeof(int32_t)); }
    return HS_OK;
}

// K2 on a tile plan; `sc` is caller-owned scratch (prepared); `after_main` (optional) is recorded right after the histogram
// kernel so that its duration can be told apart from the two small selection kernels
static int column_stats_tiled_launch(const uint8_t* d_pile, const int64_t* d_tile_off, const hs_tile_entry* d_tile_ent, int64_t total_len,
                                     hs_colstat* d_stats, int32_t min_second, int32_t* d_sel_count, int64_t* d_sel_gpos, int32_t* d_sel_depth,
                                     int32_t sel_cap, int32_t max_depth, SelectionScratch* sc, hipEvent_t after_main, hipStream_t stream,
                                     hipEvent_t after_main2 = nullptr, int64_t tile0 = 0, int64_t tile1 = -1 /* tiles [tile0, tile1) only */,
                                     int64_t g_lo = 0, int64_t g_hi = 0x7fffffffffffffffll, int32_t* d_tile_ent_sum = nullptr, bool compact = true,
                                     bool padded = false /* 256 readable bytes on both sides of the pileup */,
                                     uint2* d_sel_info = nullptr /* the stage driver: K2 also forms the leading codes and keeps only the positions the path reads */,
                                     bool* info_written = nullptr) {
    static_assert(sizeof(hs_tile_entry) == sizeof(int4), "hs_tile_entry is read as one 16-byte load");
    if (total_len <= 0) {   // nothing to count: an empty selection
        if (d_sel_count) HS_HIP(hipMemsetAsync(d_sel_count, 0, sizeof(int32_t), stream));
        if (after_main) HS_HIP(hipEventRecord(after_main, stream));
        if (after_main2) HS_HIP(hipEventRecord(after_main2, stream));
        return HS_OK;
    }
    const int64_t grid = tile1 >= 0 ? tile1 - tile0 : (total_len + 255) / 256;
    const bool full = d_stats != nullptr;
    const bool narrow = max_depth > 0 && max_depth <= 255;
    using KernelT = void (*)(const uint8_t*, const int64_t*, const int4*, int64_t, hsdev::hs_colstat_dev*, int, int32_t*, int64_t*, int32_t*, int, int64_t,
                             int64_t, int64_t, int32_t*);
    KernelT kernel = padded ? (narrow ? (full ? (KernelT)hsdev::k_column_stats_tiled<1, true, true> : (KernelT)hsdev::k_column_stats_tiled<1, false, true>)
                                      : (full ? (KernelT)hsdev::k_column_stats_tiled<2, true, true> : (KernelT)hsdev::k_column_stats_tiled<2, false, true>))
                            : (narrow ? (full ? (KernelT)hsdev::k_column_stats_tiled<1, true, false> : (KernelT)hsdev::k_column_stats_tiled<1, false, false>)
                                      : (full ? (KernelT)hsdev::k_column_stats_tiled<2, true, false> : (KernelT)hsdev::k_column_stats_tiled<2, false, false>));
    if (info_written) *info_written = false;
    if (padded && narrow && !full && d_sel_count && d_sel_info) {     // the stage driver's launch: four positions per lane, the leading codes of the selection formed on the way
        hipLaunchKernelGGL(hsdev::k_column_stats_tiled_dw, dim3((unsigned)grid), dim3(256), 0, stream, d_pile, d_tile_off, reinterpret_cast<const int4*>(d_tile_ent),
                           total_len, min_second, sc->tile_cnt.as<int32_t>(), sc->gpos.as<int64_t>(), sc->depth.as<int32_t>(), tile0, g_lo, g_hi, d_tile_ent_sum, d_sel_info);
        if (info_written) *info_written = d_sel_info != nullptr;
    } else
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, stream, d_pile, d_tile_off, reinterpret_cast<const int4*>(d_tile_ent),
                       total_len, reinterpret_cast<hsdev::hs_colstat_dev*>(d_stats), min_second, d_sel_count ? sc->tile_cnt.as<int32_t>() : nullptr,
                       d_sel_count ? sc->gpos.as<int64_t>() : nullptr, d_sel_count ? sc->depth.as<int32_t>() : nullptr, sel_cap, tile0, g_lo, g_hi,
                       d_tile_ent_sum);
    HS_HIP(hipGetLastError());
    if (after_main) HS_HIP(hipEventRecord(after_main, stream));
    if (after_main2) HS_HIP(hipEventRecord(after_main2, stream));
    if (d_sel_count && compact) return sc->finish(d_sel_count, d_sel_gpos, d_sel_depth, sel_cap, stream);
    return HS_OK;
}

int hs_column_stats_tiled(const uint8_t* d_pile, const int64_t* d_tile_off, const hs_tile_entry* d_tile_ent, int64_t total_len,
                          hs_colstat* d_stats, int32_t min_second, int32_t* d_sel_count, int64_t* d_sel_gpos, int32_t* d_sel_depth,
                          int32_t sel_cap, int32_t max_depth, void* stream) {
    if (int rc = require_device()) return rc;
    if (total_len <= 0) return HS_OK;
    SelectionScratch sc;
    if (d_sel_count) { if (int rc = sc.prepare(total_len)) return rc; }
    if (int rc = column_stats_tiled_launch(d_pile, d_tile_off, d_tile_ent, total_len, d_stats, min_second, d_sel_count, d_sel_gpos, d_sel_depth, sel_cap,
                                           max_depth, &sc, nullptr, (hipStream_t)stream)) return rc;
    if (d_sel_count) if (int rc_w = stream_wait((hipStream_t)stream)) return rc_w;   // the scratch goes back to the pool with this scope
    return HS_OK;
}

int hs_exclusive_scan_i32(const int32_t* d_in, int32_t n, int64_t* d_out, void* stream) {
    if (int rc = require_device()) return rc;
    if (n < 0) { set_error("hs_exclusive_scan_i32: negative length"); return HS_EINVAL; }
    DBuf scratch;
    if (int rc = exclusive_scan_launch(d_in, n, d_out, scratch, (hipStream_t)stream)) return rc;
    return stream_wait((hipStream_t)stream);   // the scratch goes back to the pool with this scope
}


// K4 in two steps: the lanes-as-partitions kernel on a per-contig [read][partition] table (built on the device from the
// dense state arrays), then the exact one-partition-at-a-time kernel on the few columns the first one leaves undecided
static int partition_test_launch(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const int32_t* d_col_contig,
                                 const uint8_t* d_col_k0, const uint8_t* d_col_k1, const int32_t* d_col_c1, const uint8_t* d_col_is_cand, int32_t n_cols,
                                 DBuf& b_part_off, DBuf& b_part_state_off, DBuf& b_part_state /* (filled by pk.commit below) */,
                                 const int32_t* h_part_off, const int32_t* h_contig_n_reads, int32_t n_contigs, uint8_t* d_keep, hipStream_t stream,
                                 DBuf& d_tab, DBuf& d_pres, DBuf& d_tab_off, DBuf& d_ctg_n, DBuf& d_list, UploadPack& pk, KernelClock* kc = nullptr,
                                 int64_t col_entries = 0, int64_t state_bytes = 0) {
    std::vector<int64_t> tab_off((size_t)n_contigs + 1, 0);
    std::vector<int32_t> ctg_n(h_contig_n_reads, h_contig_n_reads + n_contigs);
    int64_t max_cells = 1;
    for (int c = 0; c < n_contigs; ++c) {
        const int P = h_part_off[c + 1] - h_part_off[c];
        const int64_t cells = (int64_t)ctg_n[(size_t)c] * ((P + 15) & ~15);
        tab_off[(size_t)c + 1] = tab_off[(size_t)c] + cells;
        max_cells = std::max(max_cells, cells);
    }
    pk.add(tab_off, d_tab_off); pk.add(ctg_n, d_ctg_n);
    if (int rc = pk.commit(stream)) return rc;
    const int32_t* d_part_off = b_part_off.as<int32_t>(); const int64_t* d_part_state_off = b_part_state_off.as<int64_t>(); const int8_t* d_part_state = b_part_state.as<int8_t>();
    if (int rc = d_tab.alloc(std::max<size_t>((size_t)tab_off.back(), 64))) return rc;
    if (int rc = d_pres.alloc(std::max<size_t>((size_t)tab_off.back() / 8, 64))) return rc;      // (one 16-bit word per 16 table bytes)
    if (tab_off.back() > 0) {
        const unsigned gx = (unsigned)std::min<int64_t>((max_cells / 16 + 255) / 256, 64);      // (a thread takes a read's 16 partitions of a block)
        if (kc) { if (int rc = kc->begin(HS_K_PARTITION_TRANSPOSE, stream)) return rc; }
        hipLaunchKernelGGL(hsdev::k_partition_transpose, dim3(gx, (unsigned)n_contigs), dim3(256), 0, stream, d_part_off, d_part_state_off, d_part_state,
                           d_ctg_n.as<int32_t>(), d_tab_off.as<int64_t>(), n_contigs, d_tab.as<uint8_t>(), d_pres.as<uint16_t>());
        if (kc) { if (int rc = kc->end(state_bytes + (int64_t)tab_off.back() + (int64_t)tab_off.back() / 8, stream)) return rc; }      // the dense states in, the [read][partition] table out
    }
    // three lists: [0] = number of columns the first kernel leaves to the grouped one, [1] = number of columns that one leaves whole to the exact kernel,
    // [2] = number of (column, partition) pairs it leaves to it; [4..], [4 + n_cols..] the columns, [4 + 2 n_cols..] the pairs (room for 2 n_cols)
    if (int rc = d_list.alloc(((size_t)n_cols * 6 + 4) * 4)) return rc;
    hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, d_list.as<uint4>(), 1ll, 0u);
    int32_t* d_n_grouped = d_list.as<int32_t>(); int32_t* d_n_undecided = d_list.as<int32_t>() + 1; int32_t* d_n_pairs = d_list.as<int32_t>() + 2;
    int32_t* d_grouped = d_list.as<int32_t>() + 4; int32_t* d_undecided = d_list.as<int32_t>() + 4 + n_cols;
    int2* d_pairs = reinterpret_cast<int2*>(d_list.as<int32_t>() + 4 + 2 * (size_t)n_cols);
    const int pair_cap = 2 * n_cols;
    if (kc) { if (int rc = kc->begin(HS_K_PARTITION_LANES, stream)) return rc; }
    hipLaunchKernelGGL(hsdev::k_column_partition_lanes, dim3((n_cols + 15) / 16), dim3(256), 0, stream, d_col_off, d_col_idx, d_col_code, d_col_contig,
                       d_col_k0, d_col_k1, d_col_c1, d_col_is_cand, n_cols, d_part_off, d_ctg_n.as<int32_t>(), d_tab_off.as<int64_t>(), d_tab.as<uint8_t>(), d_keep,
                       d_grouped, d_n_grouped);
    if (kc) { if (int rc = kc->end(5 * col_entries + (int64_t)tab_off.back(), stream)) return rc; }      // the columns (idx + code) and the table, once each
    if (kc) { if (int rc = kc->begin(HS_K_PARTITION_GROUPED, stream)) return rc; }
    hipLaunchKernelGGL(hsdev::k_column_partition_grouped, dim3((unsigned)std::min((n_cols + 3) / 4, 4096)), dim3(64), 0, stream, d_col_off, d_col_idx, d_col_code,
                       d_col_contig, d_col_k0, d_col_k1, d_col_c1, d_col_is_cand, d_grouped, d_n_grouped, d_part_off, d_ctg_n.as<int32_t>(), d_tab_off.as<int64_t>(),
                       d_tab.as<uint8_t>(), d_pres.as<uint16_t>(), d_keep, d_undecided, d_n_undecided, d_pairs, d_n_pairs, pair_cap);
    if (kc) { if (int rc = kc->end(0, stream)) return rc; }      // (the columns the first kernel left open)
    if (kc) { if (int rc = kc->begin(HS_K_PARTITION_TEST, stream)) return rc; }
    hipLaunchKernelGGL(hsdev::k_column_partition_test, dim3((unsigned)std::min(n_cols, 2048)), dim3(1024), 0, stream, d_col_off, d_col_idx,
                       d_col_code, d_col_contig, d_col_k0, d_col_k1, d_col_c1, d_col_is_cand, n_cols, d_part_off, d_part_state_off,
                       d_part_state, d_keep, d_undecided, d_n_undecided);
    hipLaunchKernelGGL(hsdev::k_column_partition_pairs, dim3((unsigned)std::min((n_cols + 3) / 4, 1024)), dim3(256), 0, stream, d_col_off, d_col_idx, d_col_code, d_col_contig,
                       d_col_k0, d_col_k1, d_col_c1, d_col_is_cand, d_part_off, d_part_state_off, d_part_state, d_keep, d_pairs, d_n_pairs, pair_cap);
    HS_HIP(hipGetLastError());
    if (kc) { if (int rc = kc->end(state_bytes, stream)) return rc; }      // (the undecided columns against the dense states: a small share of them)
    return HS_OK;
}

int hs_partition_pair_distance(const int8_t* d_state, const int32_t* d_more, const int32_t* d_less, const int64_t* d_part_off, const int32_t* d_part_n,
                               const int32_t* d_pair_a, const int32_t* d_pair_b, int32_t n_pairs, int32_t threshold_p, const float* d_sigma3, int32_t* d_out,
                               void* stream) {
    if (int rc = require_device()) return rc;
    if (n_pairs <= 0) return HS_OK;
    hipLaunchKernelGGL(hsdev::k_partition_pair_distance, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_state, d_more, d_less, d_part_off,
                       d_part_n, d_pair_a, d_pair_b, n_pairs, threshold_p, d_sigma3, d_out);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

static thread_local int32_t g_k4_last_counts[4] = {0, 0, 0, 0};
int hs_column_partition_test(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code,
                             const int32_t* d_col_contig, const uint8_t* d_col_k0, const uint8_t* d_col_k1,
                             const int32_t* d_col_c1, const uint8_t* d_col_is_cand, int32_t n_cols,
                             const int32_t* d_part_off, const int64_t* d_part_state_off, const int8_t* d_part_state,
                             const int32_t* h_contig_n_reads, int32_t n_contigs, uint8_t* d_keep, void* stream) {
    if (int rc = require_device()) return rc;
    if (n_cols <= 0) return HS_OK;
    if (!h_contig_n_reads || n_contigs <= 0) { set_error("hs_column_partition_test: the number of reads of every contig is needed"); return HS_EINVAL; }
    std::vector<int32_t> h_po((size_t)n_contigs + 1);
    if (int rc = d2h_pinned(h_po.data(), d_part_off, h_po.size() * 4, (hipStream_t)stream)) return rc;
    DBuf tab, pres, tab_off, ctg_n, list, v_po, v_pso, v_ps;      // (the caller's device arrays as views)
    v_po.p = const_cast<int32_t*>(d_part_off); v_po.view = true; v_pso.p = const_cast<int64_t*>(d_part_state_off); v_pso.view = true; v_ps.p = const_cast<int8_t*>(d_part_state); v_ps.view = true;
    UploadPack pk;
    if (int rc = partition_test_launch(d_col_off, d_col_idx, d_col_code, d_col_contig, d_col_k0, d_col_k1, d_col_c1, d_col_is_cand, n_cols, v_po,
                                       v_pso, v_ps, h_po.data(), h_contig_n_reads, n_contigs, d_keep, (hipStream_t)stream, tab, pres, tab_off, ctg_n, list, pk)) return rc;
    if (int rc = stream_wait((hipStream_t)stream)) return rc;   // the table goes back to the pool with this scope
    return d2h_pinned(g_k4_last_counts, list.p, sizeof g_k4_last_counts, (hipStream_t)stream);      // (what each kernel of the chain was left with: hs_column_partition_last_counts)
}
void hs_column_partition_last_counts(int32_t out[3]) { if (out) { out[0] = g_k4_last_counts[0]; out[1] = g_k4_last_counts[1]; out[2] = g_k4_last_counts[2]; } }

}  // extern "C"

// What loop A on the device (k_loop_a) needs of the reads of every contig: their rank by start position (ties by index: the bit order of the
// partition bit sets, as hs::cv_rank_reads of the host glue), the inverse, the end of their alignment in rank order (the kernels index
// everything per read by rank), and per READ {its rank, the end of its alignment}. rec_pos / rec_end: per record of the batch.
static void loop_a_rank_reads(const int32_t* contig_rec_off, int n_contigs, const int32_t* rec_pos, const int32_t* rec_end, std::vector<int32_t>& rank_of,
                              std::vector<int32_t>& orig_of, std::vector<int32_t>& read_end, std::vector<int32_t>& rank_end) {
    const size_t n_rec = n_contigs > 0 ? (size_t)contig_rec_off[n_contigs] : 0;
    rank_of.assign(n_rec, 0); orig_of.assign(n_rec, 0); read_end.assign(n_rec, 0); rank_end.assign(n_rec * 2, 0);
    hs::hs_parallel_for(n_contigs, host_threads(), [&](int c) {
        const int r0 = contig_rec_off[c], n = contig_rec_off[c + 1] - r0;
        std::vector<int32_t> order((size_t)n);
        for (int r = 0; r < n; ++r) order[(size_t)r] = r;
        std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return rec_pos[r0 + x] != rec_pos[r0 + y] ? rec_pos[r0 + x] < rec_pos[r0 + y] : x < y; });
        for (int k = 0; k < n; ++k) { rank_of[(size_t)(r0 + order[(size_t)k])] = k; orig_of[(size_t)(r0 + k)] = order[(size_t)k]; }
        for (int k = 0; k < n; ++k) read_end[(size_t)(r0 + k)] = rec_end[r0 + order[(size_t)k]];
        for (int r = r0; r < r0 + n; ++r) { rank_end[(size_t)r * 2] = rank_of[(size_t)r]; rank_end[(size_t)r * 2 + 1] = rec_end[r]; }
    });
}

// Loop A on the device (hs_kernels_loopa.hip): the plan (which contigs, how large their partition pools), the launch sequence
// k_loop_a_offsets -> k_loop_a_prepare -> k_loop_a -> k_loop_a_scan -> k_loop_a_pack and the collection of what they leave. HipCvOps
// queues it on the candidates of its contig range; the direct test entry (hs_loop_a_test) on columns it was handed: the same calls.
struct LoopAIn {      // what the kernels read, all on the device
    const hsdev::hs_colrec_dev* rec = nullptr;      // the candidates' records (contig = index in the batch)
    const int64_t* off = nullptr;                   // their places in idx / code
    const int32_t* idx = nullptr; const uint8_t* code = nullptr;
    const int32_t* len = nullptr;                   // NULL: lengths from consecutive offsets
    const hsdev::ColumnsHeader* header = nullptr;   // n_flagged = the number of candidates
    const int32_t* ctg_n = nullptr;                 // [C] candidates of every contig of the range
    const int32_t* contig_rec_off = nullptr;        // the batch's
    const int2* rank_end = nullptr;                 // per read: {rank, alignment end}
    const int32_t* orig_of = nullptr;               // per rank: read
    int c0 = 0;                                     // first contig of the range
};
struct LoopADevice {
    struct LoopAPlan {
        std::vector<uint8_t> on_dev; std::vector<int32_t> dev_list; std::vector<int64_t> cap_off, bits_off, cnt_off;
        int w_max = 1, n_dev = 0;
    } la_plan;
    DBuf d_la_on, d_la_list, d_la_cap, d_la_bo, d_la_cno, d_la_candoff, d_la_parts, d_la_bits, d_la_cnt, d_la_meta, d_la_hdr, d_la_words, d_la_out_rec, d_la_out_bits, d_la_out_cnt, d_la_diag;
    UploadPack la_pack;
    HBuf h_la;
    bool la_launched = false;
    LoopAIn la_in;          // (of the last la_queue: a repack reads contig_rec_off and c0 again)
    static int la_grow(HBuf& h, size_t need) { if (h.cap >= need && h.p) return HS_OK; return h.alloc(need + need / 4); }
    static int la_grow(DBuf& d, size_t need) { if (d.cap >= need && d.p && !d.view) { d.bytes = need; return HS_OK; } return d.alloc(need + need / 4); }
    // the meta block the kernels leave and the host reads: [totals: partitions, span words][n_parts C][n_span C][failed C][part_base C + 1][span_base C + 1]
    struct LaLayout { size_t np, ns, nf, pb, sb, meta_bytes, rec, bits, cnt, total; int64_t cap_parts, cap_span; } lal{};
    void la_layout(int C, int64_t cap_parts, int64_t cap_span) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        lal.np = 16; lal.ns = lal.np + (size_t)C * 4; lal.nf = lal.ns + (size_t)C * 4; lal.pb = (lal.nf + (size_t)C * 4 + 7) & ~(size_t)7; lal.sb = lal.pb + ((size_t)C + 1) * 8;
        lal.meta_bytes = up(lal.sb + ((size_t)C + 1) * 8);
        lal.rec = lal.meta_bytes; lal.bits = lal.rec + up((size_t)cap_parts * sizeof(hsdev::LoopAPartition)); lal.cnt = lal.bits + up((size_t)cap_span * 24); lal.total = lal.cnt + up((size_t)cap_span * 256);
        lal.cap_parts = cap_parts; lal.cap_span = cap_span;
    }
    // the contigs of the range the device walks: those with 1 .. kmax candidates and at most 2048 reads that the host does not claim
    // (force_host, optional); the pool of each holds min(k + 8, k / pool_div + 48) partitions
    int la_make_plan(const int32_t* counts, const int32_t* n_reads, int C, int kmax, int pool_div, const uint8_t* force_host, hipStream_t stream) {
        LoopAPlan& pl = la_plan;
        pl = LoopAPlan();
        pl.on_dev.assign((size_t)C, 0); pl.cap_off.assign((size_t)C + 1, 0); pl.bits_off.assign((size_t)C + 1, 0); pl.cnt_off.assign((size_t)C + 1, 0);
        std::vector<std::pair<int64_t, int>> weight;
        for (int c = 0; c < C; ++c) {
            const int64_t k = counts[c];
            const int N = n_reads[c];
            const int W = (N + 63) >> 6;
            const bool dev = k > 0 && k <= kmax && W <= HS_LA_MAXW && !(force_host && force_host[c]);
            const int64_t cap = dev ? std::min<int64_t>(k + 8, k / pool_div + 48) : 0;
            pl.cap_off[(size_t)c + 1] = pl.cap_off[(size_t)c] + cap;
            pl.bits_off[(size_t)c + 1] = pl.bits_off[(size_t)c] + cap * 3 * W;
            pl.cnt_off[(size_t)c + 1] = pl.cnt_off[(size_t)c] + cap * W * 64;
            if (dev) { pl.on_dev[(size_t)c] = 1; pl.w_max = std::max(pl.w_max, W); weight.push_back(std::make_pair(-k, c)); }
        }
        std::sort(weight.begin(), weight.end());      // the heaviest contig first: it is what the launch waits for
        for (auto& w : weight) pl.dev_list.push_back(w.second);
        pl.n_dev = (int)pl.dev_list.size();
        if (pl.n_dev == 0) return HS_OK;
        la_pack.add(pl.on_dev, d_la_on); la_pack.add(pl.dev_list, d_la_list); la_pack.add(pl.cap_off, d_la_cap); la_pack.add(pl.bits_off, d_la_bo); la_pack.add(pl.cnt_off, d_la_cno);
        return la_pack.commit(stream);
    }
    int la_pack_launch(KernelClock& kc, hipStream_t stream) {      // the partitions packed into the form the host imports, and on their way with the meta block
        const char* meta = (const char*)d_la_meta.p;
        hipLaunchKernelGGL(hsdev::k_loop_a_pack, dim3((unsigned)la_plan.n_dev), dim3(256), 0, stream, d_la_list.as<int32_t>(), la_plan.n_dev, (const int32_t*)(meta + lal.np), la_in.c0,
                           la_in.contig_rec_off, d_la_cap.as<int64_t>(), d_la_bo.as<int64_t>(), d_la_parts.as<hsdev::LoopAPartition>(), d_la_bits.as<unsigned long long>(),
                           d_la_cnt.as<int32_t>(), (const int64_t*)(meta + lal.pb), (const int64_t*)(meta + lal.sb), (long long)lal.cap_parts, (long long)lal.cap_span,
                           d_la_out_rec.as<hsdev::LoopAPartition>(), d_la_out_bits.as<unsigned long long>(), d_la_out_cnt.as<int32_t>());
        HS_HIP(hipGetLastError());
        Shipment sh;
        sh.add(h_la.p, d_la_meta.p, lal.meta_bytes);
        sh.add_counted((char*)h_la.p + lal.rec, d_la_out_rec.p, (const long long*)meta, sizeof(hsdev::LoopAPartition), lal.cap_parts);
        sh.add_counted((char*)h_la.p + lal.bits, d_la_out_bits.p, (const long long*)meta + 1, 24, lal.cap_span);
        sh.add_counted((char*)h_la.p + lal.cnt, d_la_out_cnt.p, (const long long*)meta + 1, 256, lal.cap_span);
        if (int rc = kc.begin(HS_K_SHIP, stream)) return rc;
        if (int rc = sh.launch(stream)) return rc;
        return kc.end(0, stream);
    }
    // cap_cand: candidates the arrays of `in` hold at most; span_hint: span words to make room for (0: none known); traffic_cand: the
    // candidates the kernel clock is told of
    int la_queue(const LoopAIn& in, int C, int64_t cap_cand, int64_t span_hint, int64_t traffic_cand, KernelClock& kc, hipStream_t stream) {
        static_assert(sizeof(hs::CvPartRecord) == sizeof(hsdev::LoopAPartition), "partition record layouts differ");
        la_in = in;
        const LoopAPlan& pl = la_plan;
        const int64_t cap_parts = std::max<int64_t>(1, pl.cap_off.back());
        const int64_t cap_span = std::max<int64_t>(span_hint, std::min<int64_t>(cap_parts * pl.w_max, cap_parts * 3 + 4096));
        la_layout(C, cap_parts, cap_span);
        if (int rc = la_grow(d_la_candoff, ((size_t)C + 1) * 8)) return rc;
        if (int rc = la_grow(d_la_parts, (size_t)cap_parts * sizeof(hsdev::LoopAPartition))) return rc;
        if (int rc = la_grow(d_la_bits, std::max<size_t>(1, (size_t)pl.bits_off.back()) * 8)) return rc;
        if (int rc = la_grow(d_la_cnt, std::max<size_t>(1, (size_t)pl.cnt_off.back()) * 4)) return rc;
        if (int rc = la_grow(d_la_meta, lal.meta_bytes)) return rc;
        if (int rc = la_grow(d_la_hdr, std::max<size_t>(1, (size_t)cap_cand) * sizeof(hsdev::LoopAColumn))) return rc;
        if (int rc = la_grow(d_la_words, std::max<size_t>(1, (size_t)cap_cand) * 512)) return rc;
        if (int rc = la_grow(d_la_out_rec, (size_t)cap_parts * sizeof(hsdev::LoopAPartition))) return rc;
        if (int rc = la_grow(d_la_out_bits, (size_t)cap_span * 24)) return rc;
        if (int rc = la_grow(d_la_out_cnt, (size_t)cap_span * 256)) return rc;
        if (int rc = la_grow(h_la, lal.total)) return rc;
        if (int rc = la_grow(d_la_diag, 128)) return rc;
        char* meta = (char*)d_la_meta.p;
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(256), 0, stream, d_la_meta.as<uint4>(), (long long)(lal.meta_bytes / 16), 0u);
#ifdef HS_LA_DIAG
        hipLaunchKernelGGL(hsdev::k_fill16, dim3(1), dim3(64), 0, stream, d_la_diag.as<uint4>(), 8ll, 0u);
#endif
        hipLaunchKernelGGL(hsdev::k_loop_a_offsets, dim3(1), dim3(64), 0, stream, in.ctg_n, C, d_la_candoff.as<int64_t>());
        if (int rc = kc.begin(HS_K_ROBUST_PARTITIONS, stream)) return rc;
        hipLaunchKernelGGL(hsdev::k_loop_a_prepare, dim3((unsigned)((cap_cand + 3) / 4)), dim3(256), 0, stream, in.rec, in.off, in.idx, in.code, in.len,
                           in.header, (long long)cap_cand, in.contig_rec_off, in.rank_end, in.c0, d_la_on.as<uint8_t>(),
                           d_la_hdr.as<hsdev::LoopAColumn>(), d_la_words.as<unsigned long long>());
        hipLaunchKernelGGL(hsdev::k_loop_a, dim3((unsigned)pl.n_dev), dim3(64), 0, stream, d_la_hdr.as<hsdev::LoopAColumn>(), d_la_words.as<unsigned long long>(),
                           d_la_candoff.as<int64_t>(), d_la_list.as<int32_t>(), pl.n_dev, in.c0, in.contig_rec_off, in.orig_of,
                           d_la_cap.as<int64_t>(), d_la_bo.as<int64_t>(), d_la_cno.as<int64_t>(), d_la_parts.as<hsdev::LoopAPartition>(), d_la_bits.as<unsigned long long>(),
                           d_la_cnt.as<int32_t>(), (int32_t*)(meta + lal.np), (int32_t*)(meta + lal.ns), (int32_t*)(meta + lal.nf), d_la_diag.as<unsigned long long>());
        HS_HIP(hipGetLastError());
        if (int rc = kc.end(640 * traffic_cand, stream)) return rc;      // the columns' records and words in
        hipLaunchKernelGGL(hsdev::k_loop_a_scan, dim3(1), dim3(64), 0, stream, (const int32_t*)(meta + lal.np), (const int32_t*)(meta + lal.ns), C, (int64_t*)(meta + lal.pb),
                           (int64_t*)(meta + lal.sb), (long long*)meta);
        HS_HIP(hipGetLastError());
        if (int rc = la_pack_launch(kc, stream)) return rc;
        la_launched = true;
        return HS_OK;
    }
    // waits for what la_queue left; out views this object's pinned block. *span_words (optional): the words of all partition spans
    int la_collect(int C, hs::CvLoopAResult& out, KernelClock& kc, hipStream_t stream, int64_t* span_words) {
        out = hs::CvLoopAResult();
        if (!la_launched) return HS_OK;
        for (int attempt = 0;; ++attempt) {
            if (int rc = stream_wait(stream)) return rc;
            const long long* tot = (const long long*)h_la.p;
            if (tot[0] <= lal.cap_parts && tot[1] <= lal.cap_span) break;
            if (attempt >= 2) { set_error("loop A on the device: the packed partitions do not fit"); return HS_EINVAL; }
            // more span words than there was room for (the pools still hold every partition): packed again with room
            la_layout(C, std::max<int64_t>(lal.cap_parts, tot[0]), tot[1] + 64);
            if (int rc = la_grow(d_la_out_rec, (size_t)lal.cap_parts * sizeof(hsdev::LoopAPartition))) return rc;
            if (int rc = la_grow(d_la_out_bits, (size_t)lal.cap_span * 24)) return rc;
            if (int rc = la_grow(d_la_out_cnt, (size_t)lal.cap_span * 256)) return rc;
            if (int rc = la_grow(h_la, lal.total)) return rc;
            if (int rc = la_pack_launch(kc, stream)) return rc;
        }
        const char* h = (const char*)h_la.p;
        const long long* tot = (const long long*)h;
        const int32_t* failed = (const int32_t*)(h + lal.nf);
        out.on_device = la_plan.on_dev;
        out.failed.assign(failed, failed + C);
        out.part_base.assign((const int64_t*)(h + lal.pb), (const int64_t*)(h + lal.pb) + C + 1);
        out.rec = (const hs::CvPartRecord*)(h + lal.rec); out.bits = (const uint64_t*)(h + lal.bits); out.cnt = (const int32_t*)(h + lal.cnt);
        if (span_words) *span_words = tot[1];
        return HS_OK;
    }
};

extern "C" {

void hs_loop_a_result_destroy(hs_loop_a_result* r) {
    if (!r) return;
    std::free(r->on_device); std::free(r->failed); std::free(r->part_base); std::free(r->rec); std::free(r->state); std::free(r->more); std::free(r->less);
    delete r;
}

int hs_loop_a_test(int32_t n_contigs, const int32_t* contig_read_off, const int32_t* read_start, const int32_t* read_end, const int64_t* contig_col_off,
                   const int32_t* col_pos, const uint8_t* col_k0, const int64_t* col_off, const int32_t* col_idx, const uint8_t* col_code,
                   int32_t form, int32_t cand_bound, int32_t pool_div, int32_t light, hs_loop_a_result** out, void* stream_) {
    if (!out) { set_error("hs_loop_a_test: no place for the result"); return HS_EINVAL; }
    *out = nullptr;
    if (n_contigs < 0 || (form != 0 && form != 1) || pool_div <= 0 || !contig_read_off || !contig_col_off || !col_off) { set_error("hs_loop_a_test: bad arguments"); return HS_EINVAL; }
    const int C = n_contigs;
    const int64_t S = C ? contig_col_off[C] : 0;
    const int64_t E = S ? col_off[S] : 0;
    if (contig_read_off[0] != 0 || contig_col_off[0] != 0 || col_off[0] != 0 || S > 0x7fffffff) { set_error("hs_loop_a_test: offsets do not start at 0"); return HS_EINVAL; }
    for (int c = 0; c < C; ++c) {      // the kernels index with all of this: checked here, entry by entry
        const int N = contig_read_off[c + 1] - contig_read_off[c];
        if (N < 0 || contig_col_off[c + 1] < contig_col_off[c]) { set_error("hs_loop_a_test: offsets descend"); return HS_EINVAL; }
        for (int64_t k = contig_col_off[c]; k < contig_col_off[c + 1]; ++k) {
            if (col_off[k + 1] < col_off[k] || col_pos[k] < 0 || (k > contig_col_off[c] && col_pos[k] <= col_pos[k - 1])) { set_error("hs_loop_a_test: columns out of order"); return HS_EINVAL; }
            for (int64_t e = col_off[k]; e < col_off[k + 1]; ++e)
                if (col_idx[e] < 0 || col_idx[e] >= N || (e > col_off[k] && col_idx[e] <= col_idx[e - 1])) { set_error("hs_loop_a_test: read indices of a column out of range or order"); return HS_EINVAL; }
        }
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int n_reads_all = C ? contig_read_off[C] : 0;
    std::unique_ptr<hs_loop_a_result, void (*)(hs_loop_a_result*)> R(new hs_loop_a_result(), hs_loop_a_result_destroy);
    std::memset(R.get(), 0, sizeof(hs_loop_a_result));
    R->n_contigs = C;
    R->on_device = (int32_t*)std::calloc((size_t)C + 1, 4); R->failed = (int32_t*)std::calloc((size_t)C + 1, 4); R->part_base = (int64_t*)std::calloc((size_t)C + 1, 8);
    std::vector<hs::CvContigState*> cst((size_t)C, nullptr);
    struct Free { std::vector<hs::CvContigState*>& v; ~Free() { for (hs::CvContigState* s : v) if (s) hs::cv_state_free(s); } } free_states{cst};
    std::vector<char> has((size_t)C, 0);
    hs::ContigCvResult unused;
    for (int c = 0; c < C; ++c) {
        cst[(size_t)c] = hs::cv_state_new();
        hs::cv_phase_begin(*cst[(size_t)c], contig_read_off[c + 1] - contig_read_off[c], (int)(contig_col_off[c + 1] - contig_col_off[c]), 0.0f, unused);
    }
    if (form == 0) {      // the host's walk on the bit sets of the columns, as cv_run_range hands them to it
        for (int c = 0; c < C; ++c) {
            const int r0 = contig_read_off[c], N = contig_read_off[c + 1] - r0;
            const int64_t k0 = contig_col_off[c], n = contig_col_off[c + 1] - k0;
            std::vector<int32_t> rank_of, orig_of;
            hs::cv_rank_reads(N, read_start + r0, rank_of, orig_of);
            std::vector<hs_colrec> rec((size_t)n + 1);
            for (int64_t k = 0; k < n; ++k) { std::memset(&rec[(size_t)k], 0, sizeof(hs_colrec)); rec[(size_t)k].pos = col_pos[k0 + k]; rec[(size_t)k].contig = c; rec[(size_t)k].k0 = col_k0[k0 + k]; rec[(size_t)k].flags = HS_COL_CAND; }
            std::vector<hs::CandBits> bits((size_t)n + 1); std::vector<uint64_t> words;
            hs::cv_build_cand_bits((int)n, col_off + k0, col_idx, col_code, rank_of.data(), read_end + r0, bits.data(), words);
            words.push_back(0);
            hs::CandidateSet cs;
            cs.n = (int)n; cs.rec = rec.data(); cs.bits = bits.data(); cs.words = words.data();
            hs::cv_phase_a_host(*cst[(size_t)c], cs, read_start + r0);
            has[(size_t)c] = 1;
        }
    } else {
        if (int rc = require_device()) return rc;
        std::vector<int32_t> rank_of, orig_of, end_by_rank, rank_end;
        loop_a_rank_reads(contig_read_off, C, read_start, read_end, rank_of, orig_of, end_by_rank, rank_end);
        std::vector<int32_t> counts((size_t)C + 1, 0), n_reads((size_t)C + 1, 0), rec_off(contig_read_off, contig_read_off + C + 1);
        std::vector<hsdev::hs_colrec_dev> rec((size_t)S + 1);
        std::memset(rec.data(), 0, rec.size() * sizeof(hsdev::hs_colrec_dev));
        for (int c = 0; c < C; ++c) {
            counts[(size_t)c] = (int32_t)(contig_col_off[c + 1] - contig_col_off[c]); n_reads[(size_t)c] = contig_read_off[c + 1] - contig_read_off[c];
            for (int64_t k = contig_col_off[c]; k < contig_col_off[c + 1]; ++k) { rec[(size_t)k].pos = col_pos[k]; rec[(size_t)k].contig = c; rec[(size_t)k].k0 = col_k0[k]; rec[(size_t)k].flags = HS_COL_CAND; }
        }
        // the two layouts k_loop_a_prepare reads: packed (lengths from consecutive offsets), or "light": a place and a length per column in
        // arrays that hold the columns in another order (here: the last column first, a foreign entry between two columns)
        std::vector<int64_t> off((size_t)S + 1, 0); std::vector<int32_t> len((size_t)S + 1, 0), idx; std::vector<uint8_t> code;
        if (!light) { off.assign(col_off, col_off + S + 1); idx.assign(col_idx, col_idx + E); code.assign(col_code, col_code + E); }
        else
            for (int64_t k = S - 1; k >= 0; --k) {
                idx.push_back(0); code.push_back(255);      // (belongs to no column)
                off[(size_t)k] = (int64_t)idx.size(); len[(size_t)k] = (int32_t)(col_off[k + 1] - col_off[k]);
                idx.insert(idx.end(), col_idx + col_off[k], col_idx + col_off[k + 1]); code.insert(code.end(), col_code + col_off[k], col_code + col_off[k + 1]);
            }
        idx.push_back(0); code.push_back(0);
        if (n_reads_all == 0) { rank_end.assign(2, 0); orig_of.assign(1, 0); }
        std::vector<hsdev::ColumnsHeader> header(1);
        std::memset(header.data(), 0, sizeof(hsdev::ColumnsHeader));
        header[0].n_cols = S; header[0].n_entries = E; header[0].n_flagged = S; header[0].n_flagged_entries = E; header[0].ok = 1;
        LoopADevice la;
        KernelClock kc;
        if (int rc = la.la_make_plan(counts.data(), n_reads.data(), C, cand_bound, pool_div, nullptr, stream)) return rc;
        for (int c = 0; c < C; ++c) R->on_device[c] = la.la_plan.on_dev[(size_t)c];
        if (la.la_plan.n_dev > 0) {
            DBuf d_rec, d_off, d_idx, d_code, d_len, d_hdr, d_cn, d_ro, d_re, d_oo;
            UploadPack pk;
            pk.add(rec, d_rec); pk.add(off, d_off); pk.add(idx, d_idx); pk.add(code, d_code); pk.add(len, d_len); pk.add(header, d_hdr); pk.add(counts, d_cn); pk.add(rec_off, d_ro);
            pk.add(rank_end, d_re); pk.add(orig_of, d_oo);
            if (int rc = pk.commit(stream)) return rc;
            LoopAIn in;
            in.rec = d_rec.as<hsdev::hs_colrec_dev>(); in.off = d_off.as<int64_t>(); in.idx = d_idx.as<int32_t>(); in.code = d_code.as<uint8_t>(); in.len = light ? d_len.as<int32_t>() : nullptr;
            in.header = d_hdr.as<hsdev::ColumnsHeader>(); in.ctg_n = d_cn.as<int32_t>(); in.contig_rec_off = d_ro.as<int32_t>(); in.rank_end = d_re.as<int2>(); in.orig_of = d_oo.as<int32_t>(); in.c0 = 0;
            if (int rc = la.la_queue(in, C, S, 0, S, kc, stream)) return rc;
            hs::CvLoopAResult res;
            const int rc = la.la_collect(C, res, kc, stream, nullptr);
            const int rc_w = stream_wait(stream);      // (the uploads go back to the pool with this scope)
            kc.flush();
            if (rc) return rc;
            if (rc_w) return rc_w;
            for (int c = 0; c < C; ++c) {
                R->failed[c] = res.failed[(size_t)c];
                if (!R->on_device[c] || R->failed[c]) continue;
                const int r0 = contig_read_off[c];
                hs::cv_phase_a_import(*cst[(size_t)c], read_start + r0, (int)(res.part_base[(size_t)c + 1] - res.part_base[(size_t)c]), res.rec + res.part_base[(size_t)c], res.bits, res.cnt,
                                      rank_of.data() + r0, orig_of.data() + r0);
                has[(size_t)c] = 1;
            }
        }
    }
    // the dense export of what loop A left (a contig the device did not walk, or handed back, has no partitions here)
    int64_t P = 0, D = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t n = has[(size_t)c] ? hs::cv_loop_a_partitions(*cst[(size_t)c]) : 0;
        R->part_base[c + 1] = R->part_base[c] + n; P += n; D += n * (contig_read_off[c + 1] - contig_read_off[c]);
    }
    R->rec = (int32_t*)std::calloc((size_t)P * 9 + 1, 4); R->state = (int8_t*)std::calloc((size_t)D + 1, 1); R->more = (int32_t*)std::calloc((size_t)D + 1, 4); R->less = (int32_t*)std::calloc((size_t)D + 1, 4);
    int64_t d = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t n = R->part_base[c + 1] - R->part_base[c];
        if (n == 0) continue;
        std::vector<hs::CvPartRecord> pr((size_t)n);
        hs::cv_export_loop_a(*cst[(size_t)c], pr.data(), R->state + d, R->more + d, R->less + d);
        for (int64_t p = 0; p < n; ++p) {
            const hs::CvPartRecord& r = pr[(size_t)p];
            const int32_t v[9] = {r.left, r.right, r.n_occ, r.n_corr, r.lo, r.hi, r.reach, r.w0, r.w1};
            std::memcpy(R->rec + (R->part_base[c] + p) * 9, v, sizeof v);
        }
        d += n * (contig_read_off[c + 1] - contig_read_off[c]);
    }
    *out = R.release();
    return HS_OK;
}

// K5a: one workgroup per (contig, 4 words of its bit rows); the list of workgroups is made from the host copy of words[]
static void snp_planes_blocks(const int32_t* h_words, int n_contigs, std::vector<int32_t>& blk_c, std::vector<int32_t>& blk_w) {
    blk_c.clear(); blk_w.clear();
    for (int c = 0; c < n_contigs; ++c)
        for (int w0 = 0; w0 < h_words[c]; w0 += 4) { blk_c.push_back(c); blk_w.push_back(w0); }
}
static int snp_planes_launch(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const uint8_t* d_snp_ref,
                             const uint8_t* d_snp_alt, const int32_t* d_snp_contig, const int64_t* d_contig_snp_base, const int64_t* d_plane_off,
                             const int32_t* d_words, const int32_t* d_n_reads, const int32_t* d_blk_c, const int32_t* d_blk_w, size_t n_blocks,
                             int32_t n_snps, uint64_t* d_alt, uint64_t* d_ref, hipStream_t stream,
                             const int64_t* d_read_base = nullptr, int32_t* d_rng_lo = nullptr, int32_t* d_rng_hi = nullptr /* the words every read is present in (K5's tile ranges) */) {
    if (n_blocks == 0 || n_snps <= 0) return HS_OK;
    hipLaunchKernelGGL(hsdev::k_snp_planes, dim3((unsigned)n_blocks), dim3(HS_SP_THREADS), 0, stream, d_col_off, d_col_idx, d_col_code, d_snp_ref, d_snp_alt,
                       d_snp_contig, d_contig_snp_base, d_plane_off, d_words, d_n_reads, d_blk_c, d_blk_w, n_snps, (unsigned long long*)d_alt,
                       (unsigned long long*)d_ref, d_read_base, d_rng_lo, d_rng_hi);
    HS_HIP(hipGetLastError());
    return HS_OK;
}
int hs_snp_planes(const int64_t* d_col_off, const int32_t* d_col_idx, const uint8_t* d_col_code, const uint8_t* d_snp_ref,
                  const uint8_t* d_snp_alt, const int32_t* d_snp_contig, const int64_t* d_contig_snp_base,
                  const int64_t* d_plane_off, const int32_t* d_words, const int32_t* d_n_reads, const int32_t* h_words, int32_t n_contigs,
                  int32_t n_snps, uint64_t* d_alt, uint64_t* d_ref, void* stream) {
    if (int rc = require_device()) return rc;
    if (n_snps <= 0 || n_contigs <= 0) return HS_OK;
    if (!h_words) { set_error("hs_snp_planes: the host copy of words[] is needed"); return HS_EINVAL; }
    std::vector<int32_t> blk_c, blk_w;
    snp_planes_blocks(h_words, n_contigs, blk_c, blk_w);
    DBuf d_bc, d_bw;
    UploadPack pk;
    pk.add(blk_c, d_bc); pk.add(blk_w, d_bw);
    if (int rc = pk.commit((hipStream_t)stream)) return rc;
    if (int rc = snp_planes_launch(d_col_off, d_col_idx, d_col_code, d_snp_ref, d_snp_alt, d_snp_contig, d_contig_snp_base, d_plane_off, d_words, d_n_reads,
                                   d_bc.as<int32_t>(), d_bw.as<int32_t>(), blk_c.size(), n_snps, d_alt, d_ref, (hipStream_t)stream)) return rc;
    return stream_wait((hipStream_t)stream);   // the list goes back to the pool with this scope
}

// the upper-triangle 64 x 64 tiles of every contig's sim / diff matrices (the kernel mirrors)
static void simdiff_tiles(const std::vector<int32_t>& h_n_reads, std::vector<int32_t>& tc, std::vector<int32_t>& ti, std::vector<int32_t>& tj) {
    tc.clear(); ti.clear(); tj.clear();
    for (size_t c = 0; c < h_n_reads.size(); ++c) {
        const int nt = (h_n_reads[c] + 63) / 64;
        for (int i = 0; i < nt; ++i) for (int j = i; j < nt; ++j) { tc.push_back((int32_t)c); ti.push_back(i); tj.push_back(j); }
    }
}
static int simdiff_launch(const uint64_t* d_alt, const uint64_t* d_ref, const int64_t* d_plane_off, const int32_t* d_n_reads,
                          const int32_t* d_words, const int64_t* d_out_off, int32_t* d_sim, int32_t* d_diff, void* stream,
                          const int32_t* d_tc, const int32_t* d_ti, const int32_t* d_tj, size_t n_tiles, int es = 1 /* 2: (sim, diff) pairs, d_diff = d_sim + 1 */,
                          const int64_t* d_read_base = nullptr, const int32_t* d_orig_of = nullptr, const int32_t* d_rng_lo = nullptr, const int32_t* d_rng_hi = nullptr) {
    if (n_tiles == 0) return HS_OK;
    hipLaunchKernelGGL(hsdev::k_simdiff, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, d_alt, d_ref, d_plane_off,
                       d_n_reads, d_words, d_out_off, d_tc, d_ti, d_tj, d_sim, d_diff, es, d_read_base, d_orig_of, d_rng_lo, d_rng_hi);
    HS_HIP(hipGetLastError());
    return HS_OK;
}

int hs_simdiff(const uint64_t* d_alt, const uint64_t* d_ref, const int64_t* d_plane_off, const int32_t* d_n_reads,
               const int32_t* d_words, const int64_t* d_out_off, int32_t n_contigs, int32_t* d_sim, int32_t* d_diff,
               void* stream) {
    if (int rc = require_device()) return rc;
    if (n_contigs <= 0) return HS_OK;
    std::vector<int32_t> h_n((size_t)n_contigs);
    HS_HIP(hipMemcpy(h_n.data(), d_n_reads, sizeof(int32_t) * (size_t)n_contigs, hipMemcpyDeviceToHost));
    std::vector<int32_t> tc, ti, tj;
    simdiff_tiles(h_n, tc, ti, tj);
    DBuf a, b, c;
    UploadPack tiles;
    tiles.add(tc, a); tiles.add(ti, b); tiles.add(tj, c);
    if (int rc = tiles.commit((hipStream_t)stream)) return rc;
    if (int rc = simdiff_launch(d_alt, d_ref, d_plane_off, d_n_reads, d_words, d_out_off, d_sim, d_diff, stream, a.as<int32_t>(), b.as<int32_t>(), c.as<int32_t>(), tc.size())) return rc;
    if (int rc_w = stream_wait((hipStream_t)stream)) return rc_w;   // the tile lists die with this frame
    return HS_OK;
}


// One class of pairs (0: 8 lanes, 1: 16, 2: 32, 3: a wavefront) through the path kernel of one edlib mode and one tier of equality
// vectors (0: codes 0..3; 1 / 2: symbols and an equality table in LDS / in scratch, hs_kernels_myers.hip).
extern "C++" {
struct MyersPathArgs {
    const uint8_t* query; const int64_t* qo; const uint8_t* target; const int64_t* to; int8_t* hs; const int64_t* ho;
    unsigned long long* st; const int64_t* so; int32_t* cols; int k, task;
    int32_t *dist, *start, *end, *nloc; uint8_t* ops; const int64_t* oo; int32_t* ops_len;
    hsdev::MyersEq eq;
};
template <int MODE, int TIER>
static void myers_path_launch(const MyersPathArgs& a, int cls, const int32_t* ids, int n, hipStream_t s) {
#define HS_MYERS_GROUPED(G)                                                                                                                               \
    hipLaunchKernelGGL((hsdev::k_myers_hw_path_grouped<G, MODE, TIER>), dim3((unsigned)((n + 64 / G - 1) / (64 / G))), dim3(64), 0, s, a.query, a.qo,     \
                       a.target, a.to, ids, n, a.st, a.so, a.k, a.task, a.dist, a.start, a.end, a.nloc, a.ops, a.oo, a.ops_len, a.eq)
#define HS_MYERS_WAVE(LOCATE_ONLY)                                                                                                                        \
    hipLaunchKernelGGL((hsdev::k_myers_hw_path<MODE, TIER, LOCATE_ONLY>), dim3((unsigned)n), dim3(64), 0, s, a.query, a.qo, a.target, a.to, ids, n, a.hs, \
                       a.ho, a.st, a.so, a.cols, a.k, a.task, a.dist, a.start, a.end, a.nloc, a.ops, a.oo, a.ops_len, a.eq)
    if (cls == 0) HS_MYERS_GROUPED(8);
    else if (cls == 1) HS_MYERS_GROUPED(16);
    else if (cls == 2) HS_MYERS_GROUPED(32);
    else {
        if constexpr (TIER == 0)      // task 0 on four codes: the instantiation without steps 2 and 3 (72-79 VGPRs instead of 110)
            if (a.task == 0) { HS_MYERS_WAVE(true); return; }
        HS_MYERS_WAVE(false);
    }
#undef HS_MYERS_GROUPED
#undef HS_MYERS_WAVE
}
}  // extern "C++"

// A1 as edlibAlign(query, target, edlibNewAlignConfig(k, mode, task, NULL, 0)) (see hs_kernels_myers.hip): mode 0 NW, 1 SHW, 2 HW;
// task 0 distance, 1 locations, 2 path (d_ops required). Host offsets; the device buffers of the sequences and results are the
// caller's. d_nloc may be NULL. tier 1 / 2: the sequences are symbols 0 .. eq.n_sym - 1 and eq.mask (device) their equality
// rows (hs_edlib_align_bytes below); the scratch table of tier 2 (n_sym x 64 words per wavefront, eq.gtab: set here) counts
// against the budget.
static int edlib_align_launch(const char* who, const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off,
                              int32_t n_pairs, int32_t mode, int32_t task, int32_t k, int32_t* d_dist, int32_t* d_start, int32_t* d_end, int32_t* d_nloc,
                              uint8_t* d_ops, const int64_t* h_ops_off, int32_t* d_ops_len, void* stream, int tier = 0, hsdev::MyersEq eq = {nullptr, 0, 0, nullptr}) {
    if (int rc = require_device()) return rc;
    if (n_pairs <= 0) return HS_OK;
    if (mode < 0 || mode > 2 || task < 0 || task > 2) { set_error(std::string(who) + ": mode must be 0 (NW), 1 (SHW) or 2 (HW), task 0 (distance), 1 (locations) or 2 (path)"); return HS_EINVAL; }
    if (!h_query_off || !h_target_off || !d_dist || !d_start || !d_end || (task == 2 && (!d_ops || !h_ops_off || !d_ops_len))) { set_error(std::string(who) + ": bad arguments"); return HS_EINVAL; }
    const bool path = task == 2;
    if (k < 0) k = -1;
    std::vector<int64_t> hs_off((size_t)n_pairs + 1, 0), st_off((size_t)n_pairs + 1, 0), qo(h_query_off, h_query_off + n_pairs + 1), to(h_target_off, h_target_off + n_pairs + 1),
        oo;
    // short queries whose matrix edlib keeps whole share a wavefront: 8 / 16 / 32 lanes per pair (k_myers_hw_path_grouped); the
    // others take a wavefront each
    std::vector<int32_t> cls[4];      // 0: 8 lanes, 1: 16, 2: 32, 3: a wavefront
    const bool no_groups = std::getenv("HS_MYERS_NO_GROUPS") != nullptr;      // (diagnostic, read at every call: every pair on a wavefront of its own)
    std::vector<int64_t> need_st((size_t)n_pairs, 0), need_hs((size_t)n_pairs, 0);
    const int64_t tab_words = tier == 2 ? (int64_t)eq.n_sym * 64 : 0;      // per wavefront; counted per pair (grouped pairs share one)
    for (int i = 0; i < n_pairs; ++i) {
        const int64_t qn = qo[(size_t)i + 1] - qo[(size_t)i], tn = to[(size_t)i + 1] - to[(size_t)i];
        const int64_t nb = (qn + 63) / 64;
        const bool one_leaf = 20 * nb * tn + 8 * tn < 1024 * 1024;      // edlib.cpp:1192-1196 on the whole target: on any part of it as well
        const int c = (no_groups || nb > 32 || (path && !one_leaf)) ? 3 : nb <= 8 ? 0 : nb <= 16 ? 1 : 2;
        cls[c].push_back(i);
        need_hs[(size_t)i] = c == 3 ? ((tn + 64 + 3) & ~(int64_t)3) + 4 * (tn + 64) : 0;      // deltas (bytes) and bottoms (ints) between two passes
        need_st[(size_t)i] = path ? std::min<int64_t>(tn * nb, MY_LEAF_CELLS) * 3 : 0;      // one leaf matrix (edlib's 1-MB rule), in 8-byte words
        if (path && h_ops_off[i + 1] - h_ops_off[i] < qn + tn) { set_error(std::string(who) + ": an alignment needs room for query + target operations"); return HS_EINVAL; }
    }
    if (path) oo.assign(h_ops_off, h_ops_off + n_pairs + 1);
    // The pairs go out class by class, in chunks whose scratch (a leaf matrix per pair: up to 1.26 MB) stays within a budget: the
    // launches of a stream run one after the other, so the next chunk takes the same scratch again (HS_MYERS_SCRATCH_MB, default 16384:
    // 68 000 stage-5-sized pairs or 13 000 long ones at a time).
    const char* bud = std::getenv("HS_MYERS_SCRATCH_MB");
    const int64_t budget = std::max<int64_t>(2, bud ? std::atoll(bud) : 16384) * (1 << 20);
    struct Slice { int cls; size_t begin, end; };
    std::vector<Slice> slices;
    std::vector<int32_t> ids;
    int64_t cur_st = 0, cur_hs = 0, cur_tab = 0, max_st = 0, max_hs = 0, max_tab = 0;
    for (int c = 0; c < 4; ++c) {
        size_t begin = ids.size();
        cur_tab = 0;      // (blocks are numbered from 0 in every launch)
        for (int32_t i : cls[c]) {
            if ((cur_st > 0 || cur_hs > 0 || cur_tab > 0) && (cur_st + need_st[(size_t)i] + cur_tab + tab_words) * 8 + cur_hs + need_hs[(size_t)i] > budget) {      // the chunk is full: what came before goes out, the scratch starts over
                if (ids.size() > begin) slices.push_back(Slice{c, begin, ids.size()});
                begin = ids.size(); cur_st = 0; cur_hs = 0; cur_tab = 0;
            }
            st_off[(size_t)i] = cur_st; hs_off[(size_t)i] = cur_hs;
            cur_st += need_st[(size_t)i]; cur_hs += need_hs[(size_t)i]; cur_tab += tab_words;
            max_st = std::max(max_st, cur_st); max_hs = std::max(max_hs, cur_hs); max_tab = std::max(max_tab, cur_tab);
            ids.push_back(i);
        }
        if (ids.size() > begin) slices.push_back(Slice{c, begin, ids.size()});
    }
    DBuf d_qo, d_to, d_ho, d_so, d_oo, d_hs, d_st, d_cols, d_ids, d_tab;
    UploadPack pk;
    pk.add(qo, d_qo); pk.add(to, d_to); pk.add(hs_off, d_ho); pk.add(st_off, d_so); pk.add(ids, d_ids);
    if (path) pk.add(oo, d_oo);
    if (int rc = pk.commit((hipStream_t)stream)) return rc;
    if (int rc = d_hs.alloc(std::max<size_t>((size_t)max_hs, 1))) return rc;
    if (int rc = d_st.alloc(std::max<size_t>((size_t)max_st, 1) * 8)) return rc;
    if (int rc = d_cols.alloc(std::max<size_t>(path && !cls[3].empty() ? (size_t)(qo.back() - qo.front()) * 2 : 0, 1) * sizeof(int32_t))) return rc;      // Hirschberg's two columns
    if (int rc = d_tab.alloc(std::max<size_t>((size_t)max_tab, 1) * 8)) return rc;
    const int32_t* idp = d_ids.as<int32_t>();
    eq.gtab = d_tab.as<unsigned long long>();
    const MyersPathArgs args{d_query, d_qo.as<int64_t>(), d_target, d_to.as<int64_t>(), d_hs.as<int8_t>(), d_ho.as<int64_t>(), d_st.as<unsigned long long>(),
                             d_so.as<int64_t>(), d_cols.as<int32_t>(), k, task, d_dist, d_start, d_end, d_nloc, path ? d_ops : nullptr,
                             path ? d_oo.as<int64_t>() : nullptr, d_ops_len, eq};
    static constexpr decltype(&myers_path_launch<0, 0>) launch[3][3] = {      // [mode][tier]
        {myers_path_launch<0, 0>, myers_path_launch<0, 1>, myers_path_launch<0, 2>},
        {myers_path_launch<1, 0>, myers_path_launch<1, 1>, myers_path_launch<1, 2>},
        {myers_path_launch<2, 0>, myers_path_launch<2, 1>, myers_path_launch<2, 2>}};
    for (const Slice& sl : slices) launch[mode][tier](args, sl.cls, idp + sl.begin, (int)(sl.end - sl.begin), (hipStream_t)stream);
    HS_HIP(hipGetLastError());
    return stream_wait((hipStream_t)stream);   // the scratch goes back to the pool with this scope
}

// A1 as the stage-5 call sites use edlib: HW mode, k = -1, TASK_PATH. d_ops may be NULL (locations only: edlib's TASK_LOC).
int hs_edlib_hw_align(const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off, int32_t n_pairs,
                      int32_t* d_dist, int32_t* d_start, int32_t* d_end, uint8_t* d_ops, const int64_t* h_ops_off, int32_t* d_ops_len, void* stream) {
    return edlib_align_launch("hs_edlib_hw_align", d_query, h_query_off, d_target, h_target_off, n_pairs, 2, d_ops ? 2 : 1, -1, d_dist, d_start, d_end, nullptr,
                              d_ops, h_ops_off, d_ops_len, stream);
}

int hs_edlib_align(const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off, int32_t n_pairs, int32_t mode,
                   int32_t task, int32_t k, int32_t* d_dist, int32_t* d_start, int32_t* d_end, int32_t* d_nloc, uint8_t* d_ops, const int64_t* h_ops_off,
                   int32_t* d_ops_len, void* stream) {
    return edlib_align_launch("hs_edlib_align", d_query, h_query_off, d_target, h_target_off, n_pairs, mode, task, k, d_dist, d_start, d_end, d_nloc, d_ops,
                              h_ops_off, d_ops_len, stream);
}

// hs_edlib_align with TASK_DISTANCE and k = -1 for a caller whose offsets are on the device: they come back once, and the start
// locations the kernels write (-1 for this task) go to scratch.
int hs_edit_distance(const uint8_t* d_query, const int64_t* d_query_off, const uint8_t* d_target,
                     const int64_t* d_target_off, int32_t n_pairs, int32_t mode, int32_t* d_dist, int32_t* d_end,
                     void* stream) {
    if (int rc = require_device()) return rc;
    if (n_pairs <= 0) return HS_OK;
    if (mode < 0 || mode > 2) { set_error("hs_edit_distance: mode must be 0 (NW), 1 (SHW) or 2 (HW)"); return HS_EINVAL; }
    std::vector<int64_t> toff((size_t)n_pairs + 1), qoff((size_t)n_pairs + 1);
    HS_HIP(hipMemcpy(toff.data(), d_target_off, sizeof(int64_t) * toff.size(), hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(qoff.data(), d_query_off, sizeof(int64_t) * qoff.size(), hipMemcpyDeviceToHost));
    DBuf d_start;
    if (int rc = d_start.alloc(sizeof(int32_t) * (size_t)n_pairs)) return rc;
    const int rc = edlib_align_launch("hs_edit_distance", d_query, qoff.data(), d_target, toff.data(), n_pairs, mode, 0, -1, d_dist, d_start.as<int32_t>(), d_end,
                                      nullptr, nullptr, nullptr, nullptr, stream);      // (waits for the stream: the scratch of this scope is free after it)
    if (rc != HS_OK) stream_wait_quiet((hipStream_t)stream);      // an error after the launches: the kernels may still write d_start
    return rc;
}

// edlibAlign with additionalEqualities on raw bytes (edlib.cpp:61-92 EqualityDefinition, :357-380 buildPeq, :1422-1460
// transformSequences). Two pre-passes: which byte values the call's sequences hold (one alphabet for the whole call: a symbol a
// pair does not hold never takes part in its comparisons, so this gives what edlib's per-pair alphabet gives), then the
// sequences as symbols 0 .. A - 1 in scratch. The tier follows from A: four codes in registers (A <= 4, no equality among
// them), the LDS table (A <= 16), the scratch table (A <= 256).
int hs_edlib_align_bytes(const uint8_t* d_query, const int64_t* h_query_off, const uint8_t* d_target, const int64_t* h_target_off, int32_t n_pairs, int32_t mode,
                         int32_t task, int32_t k, const hs_equality_pair* h_equalities, int32_t n_equalities, int32_t* d_dist, int32_t* d_start, int32_t* d_end,
                         int32_t* d_nloc, uint8_t* d_ops, const int64_t* h_ops_off, int32_t* d_ops_len, void* stream) {
    if (int rc = require_device()) return rc;
    if (n_equalities < 0 || (n_equalities > 0 && !h_equalities)) { set_error("hs_edlib_align_bytes: n_equalities must be >= 0 and h_equalities given with it"); return HS_EINVAL; }
    if (n_pairs <= 0) return HS_OK;
    if (!h_query_off || !h_target_off) { set_error("hs_edlib_align_bytes: bad arguments"); return HS_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    const int64_t q0 = h_query_off[0], t0 = h_target_off[0], nq = h_query_off[n_pairs] - q0, nt = h_target_off[n_pairs] - t0;
    if (nq < 0 || nt < 0 || (nq > 0 && !d_query) || (nt > 0 && !d_target)) { set_error("hs_edlib_align_bytes: bad arguments"); return HS_EINVAL; }
    DBuf d_pres, d_map, d_mask, d_sq, d_st;
    if (int rc = d_pres.alloc(32)) return rc;
    HS_HIP(hipMemsetAsync(d_pres.p, 0, 32, st));
    if (nq + nt > 0) {
        const unsigned nblk = (unsigned)std::min<int64_t>(1024, (nq + nt + 4095) / 4096);
        hipLaunchKernelGGL(hsdev::k_myers_byte_presence, dim3(nblk), dim3(256), 0, st, d_query + q0, nq, d_target + t0, nt, d_pres.as<uint32_t>());
        HS_HIP(hipGetLastError());
    }
    uint32_t pres[8];
    if (int rc = d2h_pinned(pres, d_pres.p, sizeof pres, st)) return rc;
    std::vector<uint8_t> map(256, 0);
    int sym_of[256], A = 0;
    for (int b = 0; b < 256; ++b) { sym_of[b] = ((pres[b >> 5] >> (b & 31)) & 1u) ? A++ : -1; if (sym_of[b] >= 0) map[(size_t)b] = (uint8_t)sym_of[b]; }
    if (A == 0) A = 1;      // (every sequence empty: nothing is compared)
    const int words = A <= 32 ? 1 : (A + 31) / 32;
    std::vector<uint32_t> mask((size_t)A * words, 0u);
    for (int a = 0; a < A; ++a) mask[(size_t)a * words + (a >> 5)] |= 1u << (a & 31);
    bool extra = false;
    for (int i = 0; i < n_equalities; ++i) {
        const int a = sym_of[h_equalities[i].first], b = sym_of[h_equalities[i].second];
        if (a < 0 || b < 0 || a == b) continue;      // edlib.cpp:75-85: a pair naming a byte outside the alphabet is ignored
        mask[(size_t)a * words + (b >> 5)] |= 1u << (b & 31); mask[(size_t)b * words + (a >> 5)] |= 1u << (a & 31);
        extra = true;
    }
    const int tier = (A <= 4 && !extra) ? 0 : A <= 16 ? 1 : 2;
    UploadPack pk;
    pk.add(map, d_map); pk.add(mask, d_mask);
    if (int rc = pk.commit(st)) return rc;
    if (int rc = d_sq.alloc((size_t)std::max<int64_t>(nq, 1))) return rc;
    if (int rc = d_st.alloc((size_t)std::max<int64_t>(nt, 1))) return rc;
    if (nq > 0) hipLaunchKernelGGL(hsdev::k_myers_compact, dim3((unsigned)std::min<int64_t>(4096, (nq + 1023) / 1024)), dim3(256), 0, st, d_query + q0, nq, d_map.as<uint8_t>(), d_sq.as<uint8_t>());
    if (nt > 0) hipLaunchKernelGGL(hsdev::k_myers_compact, dim3((unsigned)std::min<int64_t>(4096, (nt + 1023) / 1024)), dim3(256), 0, st, d_target + t0, nt, d_map.as<uint8_t>(), d_st.as<uint8_t>());
    HS_HIP(hipGetLastError());
    std::vector<int64_t> qo((size_t)n_pairs + 1), to((size_t)n_pairs + 1);
    for (int i = 0; i <= n_pairs; ++i) { qo[(size_t)i] = h_query_off[i] - q0; to[(size_t)i] = h_target_off[i] - t0; }
    const int rc = edlib_align_launch("hs_edlib_align_bytes", d_sq.as<uint8_t>(), qo.data(), d_st.as<uint8_t>(), to.data(), n_pairs, mode, task, k, d_dist, d_start,
                                      d_end, d_nloc, d_ops, h_ops_off, d_ops_len, stream, tier, hsdev::MyersEq{d_mask.as<uint32_t>(), A, words, nullptr});      // (waits for the stream: the scratch of this scope is free after it)
    if (rc != HS_OK) stream_wait_quiet(st);      // refused arguments: the pre-passes still run on this scope's scratch
    return rc;
}

// edlibAlignmentToCigar (edlib.cpp:299-349): runs of equal move characters, count then character; STANDARD writes '=' and 'X' as 'M'.
int hs_alignment_to_cigar(const uint8_t* ops, int32_t n_ops, int32_t format, char** out) {
    if (!out || n_ops < 0 || (n_ops > 0 && !ops) || format < 0 || format > 1) { set_error("hs_alignment_to_cigar: bad arguments"); return HS_EINVAL; }
    const char* sym = format == 0 ? "MIDM" : "=IDX";
    std::string s;
    for (int32_t i = 0; i < n_ops;) {
        if (ops[i] > 3) { set_error("hs_alignment_to_cigar: move code above 3 at " + std::to_string(i)); return HS_EINVAL; }
        int32_t j = i + 1;
        while (j < n_ops && ops[j] <= 3 && sym[ops[j]] == sym[ops[i]]) ++j;
        s += std::to_string(j - i);
        s += sym[ops[i]];
        i = j;
    }
    char* p = static_cast<char*>(std::malloc(s.size() + 1));
    if (!p) { set_error("hs_alignment_to_cigar: out of host memory"); return HS_EINVAL; }
    std::memcpy(p, s.c_str(), s.size() + 1);
    *out = p;
    return HS_OK;
}

