// hs_capi_polish.inc -- the polisher's inputs (create_new_contigs.cpp:358-521) on the resident batch: the host side of
// hs_kernels_polish.hip. The host lists the (interval, read) tasks, k_polish_cut walks them, the sizes come back (the one host
// wait the sizes cost), the host forms the groups and 64-bit offsets, and k_polish_gather / k_polish_cigar fill the output in
// rounds whose device scratch stays within HS_POLISH_CHUNK_MB. A round ends in the downloads of hs_polish_inputs or, for hs_polish_haplotypes
// (hs_capi_consensus.inc), in a sink that works on the round's buffers where they are.

namespace {

struct PolishBundle { int32_t contig, interval, start, end, group, left, right, ovl, ovr; };
struct PolishIntervalBounds { int32_t left, right, ovl, ovr; };

// create_new_contigs.cpp:371-375
PolishIntervalBounds polish_bounds(int L, int start, int end) {
    PolishIntervalBounds b;
    b.ovl = std::min(start, 150);
    b.ovr = std::max(0, std::min(L - end - 1, 150));
    b.left = std::max(0, start - b.ovl);
    b.right = std::min(L - 1, end + b.ovr + 1);
    return b;
}
// std::string(L bytes).substr(pos, (size_t)count): the range it yields. A negative int count is npos; pos beyond the string makes the
// reference throw -- an empty range here
void polish_substr(int64_t L, int64_t pos, int64_t count, int64_t& p, int64_t& n) {
    p = pos; n = 0;
    if (pos < 0 || pos > L) { p = 0; return; }
    n = count < 0 ? L - pos : std::min(count, L - pos);
}
// toPolish, :517-519: three pieces of the backbone
void polish_backbone_ranges(int L, int start, int end, const PolishIntervalBounds& b, int64_t pos[3], int64_t len[3]) {
    polish_substr(L, std::max(0, start - b.ovl), std::min(b.ovl, start), pos[0], len[0]);
    polish_substr(L, start, end - start, pos[1], len[1]);
    polish_substr(L, end, std::min(b.ovr + 1, L - end - 1), pos[2], len[2]);
}

// a large device array into pageable host memory, 64 MB of pinned staging at a time
int polish_download(void* dst, const void* d, size_t n, hipStream_t s) {
    const size_t step = (size_t)64 << 20;
    for (size_t o = 0; o < n; o += step)
        if (int rc = d2h_pinned((char*)dst + o, (const char*)d + o, std::min(step, n - o), s)) return rc;
    return HS_OK;
}

struct PolishTimer {   // HIP events around a group of launches, summed when the stream has drained
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    hipStream_t s;
    explicit PolishTimer(hipStream_t st) : s(st) {}
    ~PolishTimer() { for (auto& e : ev) for (hipEvent_t x : {e.first, e.second}) if (x) EventPair::cache().push_back(x); }      // (recycled, as every timing event of the library)
    void begin() { hipEvent_t a = nullptr, b = nullptr; (void)EventPair::get(&a); (void)EventPair::get(&b); ev.push_back({a, b}); (void)ev_rec(a, s); }
    void end() { (void)ev_rec(ev.back().second, s); }
    double ms() { double t = 0; for (auto& e : ev) { float x = 0; if (hipEventElapsedTime(&x, e.first, e.second) == hipSuccess) t += x; } return t; }
};

struct BytesMoved { int64_t up = 0, down = 0; };      // what a call sent to the device and fetched from it

// what the host needs of the records: strand, op ranges, reads, the reads' ranges (the batch keeps them on the device): one shipment and one
// host wait on the batch's first polishing call, none after it
int polish_host_recs(const hs_cv_batch* b, BytesMoved* moved) {
    std::lock_guard<std::mutex> g(b->polish_mu);
    if (b->polish_have) return HS_OK;
    const size_t n_rec = (size_t)b->n_rec, n_reads = (size_t)b->n_reads;
    const size_t part[4] = {n_rec, (n_rec + 1) * 8, (n_reads + 1) * 8, n_rec * 4};
    const void* src[4] = {b->rec_strand.p, b->rec_cig_off.p, b->read_off.p, b->rec_read.p};
    size_t at[4], total = 0;
    for (int k = 0; k < 4; ++k) { at[k] = total; total += (part[k] + 31) & ~(size_t)15; }
    HBuf h;
    if (int rc = h.alloc(total + 16)) return rc;
    Shipment sh;
    for (int k = 0; k < 4; ++k) if (k == 2 || n_rec) sh.add((char*)h.p + at[k], src[k], part[k]);
    if (int rc = sh.launch(nullptr)) return rc;
    if (int rc = stream_wait(nullptr)) return rc;
    b->h_rec_strand.assign(n_rec, 0); b->h_rec_cig_off.assign(n_rec + 1, 0); b->h_read_off.assign(n_reads + 1, 0); b->h_rec_read.assign(n_rec, 0);
    void* dst[4] = {b->h_rec_strand.data(), b->h_rec_cig_off.data(), b->h_read_off.data(), b->h_rec_read.data()};
    for (int k = 0; k < 4; ++k) if (k == 2 || n_rec) std::memcpy(dst[k], (char*)h.p + at[k], part[k]);
    if (moved) moved->down += (int64_t)(part[0] + part[1] + part[2] + part[3]);
    b->polish_have = true;
    return HS_OK;
}

// a round of polish_inputs_core as its sink sees it: the bundles [b0, b1) of the call's tables (host arrays over all bundles and pieces of the
// call) and the round's device buffers, which begin where the round's first piece and first bundle begin
struct PolishRound {
    int64_t b0, b1;
    const int64_t *backbone_off, *piece_off, *base_off, *cig_off;
    const int32_t *ovl, *ovr, *sam, *flags;
    const uint8_t *d_bases, *d_bb;
    const uint32_t* d_cig;
    hipStream_t st;
};
typedef std::function<int(const PolishRound&)> PolishSink;

// sink == nullptr: the round's bases, backbones and CIGAR words come down into the result (hs_polish_inputs). With a sink they stay on the
// device, the sink works on them there, and the result's backbone, bases and cigar are NULL.
int polish_inputs_core(hs_cv_batch* b, int c0, int c1, const std::vector<std::vector<hs::LabelledInterval>>& ivs, const std::vector<uint8_t>& has,
                       bool polish_everything, hs_polish_result** out, const PolishSink* sink = nullptr, BytesMoved* moved = nullptr) {
    using namespace hsdev;
    hipStream_t st = nullptr;
    const int n_rec = b->n_rec;
    if (int rc = polish_host_recs(b, moved)) return rc;
    const std::vector<uint8_t>& rec_strand = b->h_rec_strand;
    const std::vector<int64_t>&rec_cig_off = b->h_rec_cig_off, &read_off = b->h_read_off;
    const std::vector<int32_t>& rec_read = b->h_rec_read;

    // ---- the intervals of the call and their tasks: every read with a label above -1 (:383-384)
    struct Interval { int32_t contig, index, start, end; PolishIntervalBounds bd; int64_t task0, task1; const std::vector<int>* lab; };
    std::vector<Interval> intervals;
    std::vector<std::vector<int>> default_labels;      // :249-251
    default_labels.reserve((size_t)(c1 - c0));
    std::vector<PolishTask> tasks;
    std::vector<int32_t> slot_of_rec((size_t)n_rec, -1), recs;
    for (int c = c0; c < c1; ++c) {
        const int L = (int)(b->contig_off[(size_t)c + 1] - b->contig_off[(size_t)c]);
        const int r0 = b->contig_rec_off[(size_t)c], n = b->contig_rec_off[(size_t)c + 1] - r0;
        const std::vector<hs::LabelledInterval>* list = &ivs[(size_t)c];
        if (!has[(size_t)c]) {
            if (!polish_everything) continue;
            default_labels.emplace_back((size_t)n, 0);
        }
        const int n_iv = has[(size_t)c] ? (int)list->size() : 1;
        for (int k = 0; k < n_iv; ++k) {
            Interval iv;
            iv.contig = c; iv.index = k;
            if (has[(size_t)c]) { iv.start = (*list)[(size_t)k].first.first; iv.end = (*list)[(size_t)k].first.second; iv.lab = &(*list)[(size_t)k].second; }
            else { iv.start = 0; iv.end = L; iv.lab = &default_labels.back(); }
            if ((int)iv.lab->size() != n) { set_error("hs_polish_inputs: an interval does not hold one label per record"); return HS_EINVAL; }
            iv.bd = polish_bounds(L, iv.start, iv.end);
            iv.task0 = (int64_t)tasks.size();
            for (int r = 0; r < n; ++r)
                if ((*iv.lab)[(size_t)r] > -1) {
                    tasks.push_back(PolishTask{r0 + r, iv.bd.left, iv.bd.right, 0});
                    if (slot_of_rec[(size_t)(r0 + r)] < 0) { slot_of_rec[(size_t)(r0 + r)] = (int32_t)recs.size(); recs.push_back(r0 + r); }
                }
            iv.task1 = (int64_t)tasks.size();
            intervals.push_back(iv);
        }
    }
    if (tasks.size() > (size_t)0x7fffffff - 8) { set_error("hs_polish_inputs: too many (interval, read) tasks for one call; split the contig range"); return HS_EINVAL; }
    const int n_tasks = (int)tasks.size(), n_slots = (int)recs.size();

    // ---- the cursor table of the records that take part, then the walk
    std::vector<int64_t> chunk_off((size_t)n_slots + 1, 0);
    for (int i = 0; i < n_slots; ++i) {
        const int64_t ops = rec_cig_off[(size_t)recs[(size_t)i] + 1] - rec_cig_off[(size_t)recs[(size_t)i]];
        chunk_off[(size_t)i + 1] = chunk_off[(size_t)i] + (ops + 63) / 64;
    }
    std::vector<int32_t> cut((size_t)n_tasks * PC_SLOTS);
    PolishTimer t_scan(st), t_cut(st), t_gather(st), t_cigar(st);
    int64_t cut_ops = 0;
    {
        DBuf d_tasks, d_slot, d_recs, d_chunk_off, d_tab, d_cut;
        UploadPack pk;
        pk.add(tasks, d_tasks); pk.add(slot_of_rec, d_slot); pk.add(recs, d_recs); pk.add(chunk_off, d_chunk_off);
        if (moved) moved->up += (int64_t)pk.total;
        if (int rc = pk.commit(st)) return rc;
        if (int rc = d_tab.alloc(std::max<size_t>((size_t)chunk_off.back(), 1) * 2 * sizeof(int32_t))) return rc;
        if (int rc = d_cut.alloc(std::max<size_t>(cut.size(), 1) * sizeof(int32_t))) return rc;
        if (n_slots) {
            t_scan.begin();
            hipLaunchKernelGGL(k_polish_scan, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, st, d_recs.as<int32_t>(), n_slots, b->d_rec_pos.as<int32_t>(),
                               b->rec_cig_off.as<int64_t>(), b->cigar.as<uint32_t>(), d_chunk_off.as<int64_t>(), d_tab.as<int32_t>());
            t_scan.end();
        }
        if (n_tasks) {
            t_cut.begin();
            hipLaunchKernelGGL(k_polish_cut, dim3((unsigned)((n_tasks + 3) / 4)), dim3(256), 0, st, d_tasks.as<PolishTask>(), n_tasks, d_slot.as<int32_t>(),
                               b->d_rec_pos.as<int32_t>(), b->rec_read.as<int32_t>(), b->read_off.as<int64_t>(), b->rec_cig_off.as<int64_t>(),
                               b->cigar.as<uint32_t>(), d_chunk_off.as<int64_t>(), d_tab.as<int32_t>(), d_cut.as<int32_t>());
            t_cut.end();
        }
        HS_HIP(hipGetLastError());
        if (int rc = polish_download(cut.data(), d_cut.p, cut.size() * sizeof(int32_t), st)) return rc;      // the host wait of the call
        if (moved) moved->down += (int64_t)(cut.size() * sizeof(int32_t));
    }

    // ---- groups and bundles (:478-506, :523), pieces in (bundle, record) order
    std::vector<PolishBundle> bundles;
    std::vector<int64_t> piece_off{0}, base_off{0}, cig_off{0}, backbone_off{0};
    std::vector<int32_t> piece_rec, piece_rs, piece_re, piece_sam, piece_flags, piece_task, dropped;
    for (const Interval& iv : intervals) {
        const int r0 = b->contig_rec_off[(size_t)iv.contig];
        const int L = (int)(b->contig_off[(size_t)iv.contig + 1] - b->contig_off[(size_t)iv.contig]);
        std::vector<std::pair<int, int64_t>> alive;      // (label, task) of the reads that stay
        std::vector<int> parts;                          // existingparts
        for (int64_t t = iv.task0; t < iv.task1; ++t) {
            const int32_t* o = &cut[(size_t)t * PC_SLOTS];
            const int r = tasks[(size_t)t].rec - r0;
            parts.push_back((*iv.lab)[(size_t)r]);
            cut_ops += 64 * (int64_t)o[PC_CHUNKS];
            if (o[PC_FLAGS] & POLISH_DROPPED) { dropped.push_back(iv.contig); dropped.push_back(iv.index); dropped.push_back(r); continue; }
            alive.push_back({(*iv.lab)[(size_t)r], t});
        }
        std::sort(parts.begin(), parts.end());
        parts.erase(std::unique(parts.begin(), parts.end()), parts.end());
        std::stable_sort(alive.begin(), alive.end(), [](const std::pair<int, int64_t>& x, const std::pair<int, int64_t>& y) { return x.first < y.first; });
        int n_clusters = 0;
        for (size_t i = 0; i < alive.size(); ++i) n_clusters += i == 0 || alive[i].first != alive[i - 1].first;
        if (parts.empty() && !iv.lab->empty()) parts.push_back(-1);      // :493-499: the interval defaults back to the consensus
        if (!(n_clusters > 1 || polish_everything)) continue;           // :523
        int64_t bp[3], bl[3];
        polish_backbone_ranges(L, iv.start, iv.end, iv.bd, bp, bl);
        size_t a = 0;
        for (int g : parts) {
            bundles.push_back(PolishBundle{iv.contig, iv.index, iv.start, iv.end, g, iv.bd.left, iv.bd.right, iv.bd.ovl, iv.bd.ovr});
            backbone_off.push_back(backbone_off.back() + bl[0] + bl[1] + bl[2]);
            for (; a < alive.size() && alive[a].first == g; ++a) {
                const int64_t t = alive[a].second;
                const int32_t* o = &cut[(size_t)t * PC_SLOTS];
                piece_task.push_back((int32_t)t);
                piece_rec.push_back(tasks[(size_t)t].rec - r0);
                piece_rs.push_back(o[PC_READ_START]); piece_re.push_back(o[PC_READ_END]); piece_sam.push_back(o[PC_SAM_POS]);
                piece_flags.push_back(o[PC_FLAGS]);
                base_off.push_back(base_off.back() + o[PC_LEN]);
                cig_off.push_back(cig_off.back() + o[PC_N_OPS]);
            }
            piece_off.push_back((int64_t)piece_rec.size());
        }
    }
    const int64_t n_bundles = (int64_t)bundles.size(), n_pieces = (int64_t)piece_rec.size();

    hs_polish_result* res = static_cast<hs_polish_result*>(std::calloc(1, sizeof(hs_polish_result)));
    if (!res) { set_error("hs_polish_inputs: out of host memory"); return HS_EINVAL; }
    std::unique_ptr<hs_polish_result, void (*)(hs_polish_result*)> guard(res, hs_polish_result_destroy);
    res->n_bundles = n_bundles; res->n_pieces = n_pieces; res->n_dropped = (int64_t)dropped.size() / 3;
    if (!sink) {
        res->backbone = static_cast<uint8_t*>(std::malloc((size_t)std::max<int64_t>(backbone_off.back(), 1)));
        res->bases = static_cast<uint8_t*>(std::malloc((size_t)std::max<int64_t>(base_off.back(), 1)));
        res->cigar = static_cast<uint32_t*>(std::malloc((size_t)std::max<int64_t>(cig_off.back(), 1) * sizeof(uint32_t)));
        if (!res->backbone || !res->bases || !res->cigar) { set_error("hs_polish_inputs: out of host memory"); return HS_EINVAL; }
    }
    std::vector<int32_t> bundle_ovl, bundle_ovr;      // (what a sink reads of the bundles)
    if (sink) for (const PolishBundle& bu : bundles) { bundle_ovl.push_back(bu.ovl); bundle_ovr.push_back(bu.ovr); }

    // ---- rounds over bundle ranges that end with a contig: gather + CIGAR into scratch, then down
    const char* bud = std::getenv("HS_POLISH_CHUNK_MB");
    const int64_t budget = std::max<int64_t>(1, bud ? std::atoll(bud) : 1024) * (1 << 20);
    int64_t n_rounds = 0;
    for (int64_t b0 = 0; b0 < n_bundles;) {
        int64_t b1 = b0;
        auto bytes_of = [&](int64_t lo, int64_t hi) {
            return (backbone_off[(size_t)hi] - backbone_off[(size_t)lo]) + (base_off[(size_t)piece_off[(size_t)hi]] - base_off[(size_t)piece_off[(size_t)lo]]) +
                   4 * (cig_off[(size_t)piece_off[(size_t)hi]] - cig_off[(size_t)piece_off[(size_t)lo]]);
        };
        while (b1 < n_bundles) {      // whole contigs; at least one
            int64_t e = b1;
            while (e < n_bundles && bundles[(size_t)e].contig == bundles[(size_t)b1].contig) ++e;
            if (b1 > b0 && bytes_of(b0, e) > budget) break;
            b1 = e;
        }
        ++n_rounds;
        const int64_t p0 = piece_off[(size_t)b0], p1 = piece_off[(size_t)b1];
        const int64_t base0 = base_off[(size_t)p0], cig0 = cig_off[(size_t)p0], bb0 = backbone_off[(size_t)b0];
        const int64_t n_base = base_off[(size_t)p1] - base0, n_cig = cig_off[(size_t)p1] - cig0, n_bb = backbone_off[(size_t)b1] - bb0;
        std::vector<PolishPiece> rp, bpieces;
        std::vector<PolishSlice> rs, bs;
        std::vector<PolishCigTask> ct;
        auto add_slices = [](std::vector<PolishSlice>& sl, int32_t piece, int64_t off, int64_t len) {
            if (len <= 0) return;
            for (int64_t w = off >> 12; w <= (off + len - 1) >> 12; ++w) sl.push_back(PolishSlice{piece, (int32_t)w});
        };
        for (int64_t p = p0; p < p1; ++p) {
            const int32_t t = piece_task[(size_t)p];
            const int32_t* o = &cut[(size_t)t * PC_SLOTS];
            const int rec = tasks[(size_t)t].rec, rd = rec_read[(size_t)rec];
            const int64_t rlen = read_off[(size_t)rd + 1] - read_off[(size_t)rd];
            const bool rev = rec_strand[(size_t)rec] == 0;      // :454-456
            const int64_t len = base_off[(size_t)p + 1] - base_off[(size_t)p];
            rp.push_back(PolishPiece{base_off[(size_t)p] - base0, rev ? read_off[(size_t)rd] + rlen - 1 - o[PC_READ_START] : read_off[(size_t)rd] + o[PC_READ_START],
                                     (int32_t)len, rev ? 1 : 0});
            add_slices(rs, (int32_t)(p - p0), base_off[(size_t)p] - base0, len);
            if (cig_off[(size_t)p + 1] > cig_off[(size_t)p])
                ct.push_back(PolishCigTask{rec, o[PC_OP_FIRST], o[PC_OFF_FIRST], o[PC_OP_LAST], o[PC_OFF_LAST], o[PC_N_OPS], cig_off[(size_t)p] - cig0});
        }
        for (int64_t k = b0; k < b1; ++k) {
            const PolishBundle& bu = bundles[(size_t)k];
            const int L = (int)(b->contig_off[(size_t)bu.contig + 1] - b->contig_off[(size_t)bu.contig]);
            int64_t bp[3], bl[3], o = backbone_off[(size_t)k] - bb0;
            polish_backbone_ranges(L, bu.start, bu.end, PolishIntervalBounds{bu.left, bu.right, bu.ovl, bu.ovr}, bp, bl);
            for (int j = 0; j < 3; ++j) {
                if (bl[j] <= 0) continue;
                bpieces.push_back(PolishPiece{o, b->contig_off[(size_t)bu.contig] + bp[j], (int32_t)bl[j], 0});
                add_slices(bs, (int32_t)bpieces.size() - 1, o, bl[j]);
                o += bl[j];
            }
        }
        if (rs.size() > (size_t)0x7fffffff || bs.size() > (size_t)0x7fffffff) { set_error("hs_polish_inputs: a round is too large; lower HS_POLISH_CHUNK_MB"); return HS_EINVAL; }
        DBuf d_rp, d_rs, d_bp, d_bs, d_ct, d_bases, d_bb, d_cig;
        UploadPack pk;
        pk.add(rp, d_rp); pk.add(rs, d_rs); pk.add(bpieces, d_bp); pk.add(bs, d_bs); pk.add(ct, d_ct);
        if (moved) moved->up += (int64_t)pk.total;
        if (int rc = pk.commit(st)) return rc;
        if (int rc = d_bases.alloc((size_t)n_base + 16)) return rc;
        if (int rc = d_bb.alloc((size_t)n_bb + 16)) return rc;
        if (int rc = d_cig.alloc(((size_t)n_cig + 4) * sizeof(uint32_t))) return rc;
        t_gather.begin();
        if (!rs.empty())
            hipLaunchKernelGGL(k_polish_gather, dim3((unsigned)rs.size()), dim3(256), 0, st, d_rp.as<PolishPiece>(), d_rs.as<PolishSlice>(), b->read_ptr(), d_bases.as<uint8_t>());
        if (!bs.empty())
            hipLaunchKernelGGL(k_polish_gather, dim3((unsigned)bs.size()), dim3(256), 0, st, d_bp.as<PolishPiece>(), d_bs.as<PolishSlice>(), b->contig_ptr(), d_bb.as<uint8_t>());
        t_gather.end();
        t_cigar.begin();
        if (!ct.empty())
            hipLaunchKernelGGL(k_polish_cigar, dim3((unsigned)((ct.size() + 3) / 4)), dim3(256), 0, st, d_ct.as<PolishCigTask>(), (int)ct.size(), b->rec_cig_off.as<int64_t>(),
                               b->cigar.as<uint32_t>(), d_cig.as<uint32_t>());
        t_cigar.end();
        HS_HIP(hipGetLastError());
        if (sink) {      // the pieces stay where they are
            const PolishRound round{b0, b1, backbone_off.data(), piece_off.data(), base_off.data(), cig_off.data(), bundle_ovl.data(), bundle_ovr.data(), piece_sam.data(),
                                    piece_flags.data(), d_bases.as<uint8_t>(), d_bb.as<uint8_t>(), d_cig.as<uint32_t>(), st};
            if (int rc = (*sink)(round)) return rc;
        } else {
            if (int rc = polish_download(res->bases + base0, d_bases.p, (size_t)n_base, st)) return rc;
            if (int rc = polish_download(res->backbone + bb0, d_bb.p, (size_t)n_bb, st)) return rc;
            if (int rc = polish_download(res->cigar + cig0, d_cig.p, (size_t)n_cig * sizeof(uint32_t), st)) return rc;
            if (moved) moved->down += n_base + n_bb + n_cig * 4;
        }
        b0 = b1;
    }
    if (int rc = stream_wait_quiet(st)) return rc;

    std::vector<int32_t> f[9];
    for (const PolishBundle& bu : bundles) {
        const int32_t v[9] = {bu.contig, bu.interval, bu.start, bu.end, bu.group, bu.left, bu.right, bu.ovl, bu.ovr};
        for (int j = 0; j < 9; ++j) f[j].push_back(v[j]);
    }
    res->bundle_contig = malloc_copy(f[0]); res->bundle_interval = malloc_copy(f[1]); res->bundle_start = malloc_copy(f[2]);
    res->bundle_end = malloc_copy(f[3]); res->bundle_group = malloc_copy(f[4]); res->bundle_left_to_polish = malloc_copy(f[5]);
    res->bundle_right_to_polish = malloc_copy(f[6]); res->bundle_overhang_left = malloc_copy(f[7]); res->bundle_overhang_right = malloc_copy(f[8]);
    res->backbone_off = malloc_copy(backbone_off); res->piece_off = malloc_copy(piece_off);
    res->piece_rec = malloc_copy(piece_rec); res->piece_read_start = malloc_copy(piece_rs); res->piece_read_end = malloc_copy(piece_re);
    res->piece_sam_pos = malloc_copy(piece_sam); res->piece_flags = malloc_copy(piece_flags);
    res->base_off = malloc_copy(base_off); res->cig_off = malloc_copy(cig_off); res->dropped = malloc_copy(dropped);
    res->t_scan_ms = t_scan.ms(); res->t_cut_ms = t_cut.ms(); res->t_gather_ms = t_gather.ms(); res->t_cigar_ms = t_cigar.ms();
    res->n_tasks = n_tasks; res->n_rounds = n_rounds; res->cut_ops_read = cut_ops;
    *out = guard.release();
    return HS_OK;
}

}  // namespace

void hs_polish_result_destroy(hs_polish_result* r) {
    if (!r) return;
    void* p[] = {r->bundle_contig, r->bundle_interval, r->bundle_start, r->bundle_end, r->bundle_group, r->bundle_left_to_polish, r->bundle_right_to_polish,
                 r->bundle_overhang_left, r->bundle_overhang_right, r->backbone_off, r->backbone, r->piece_off, r->piece_rec, r->piece_read_start, r->piece_read_end,
                 r->piece_sam_pos, r->piece_flags, r->base_off, r->bases, r->cig_off, r->cigar, r->dropped};
    for (void* q : p) std::free(q);
    std::free(r);
}

int hs_polish_inputs(hs_cv_batch* b, int32_t c0, int32_t c1, const int64_t* win_off, const int32_t* win_start, const int32_t* win_end,
                     const int64_t* label_off, const int32_t* labels, const uint8_t* contig_has_snps, int32_t polish_everything, hs_polish_result** out) {
    if (int rc = require_device()) return rc;
    if (!b || !out || !win_off || !label_off || c0 < 0 || c1 < c0 || c1 > b->n_contigs) { set_error("hs_polish_inputs: bad arguments"); return HS_EINVAL; }
    if (int rc = bind_device(b->device)) return rc;
    try {
        if (int rc = polish_host_recs(b, nullptr)) return rc;
        std::vector<std::vector<hs::LabelledInterval>> ivs;
        std::vector<uint8_t> has;
        if (int rc = hs::polish_intervals_from_labels(b->n_contigs, b->contig_rec_off.data(), b->h_rec_read.data(), win_off, win_start, win_end, label_off, labels,
                                                      contig_has_snps, ivs, has))
            return rc;
        return polish_inputs_core(b, c0, c1, ivs, has, polish_everything != 0, out);
    } catch (const std::exception& e) { set_error(std::string("hs_polish_inputs: ") + e.what()); return HS_EINVAL; }
}

int hs_polish_inputs_from_files(const char* gfa, const char* reads, const char* sam, const char* gro, int32_t polish_everything, const char* out_path,
                                int32_t n_threads) {
    if (int rc = require_device()) return rc;
    if (!gfa || !reads || !sam || !gro || !out_path) { set_error("hs_polish_inputs_from_files: null path"); return HS_EINVAL; }
    // HS_HAPLOTYPES=1: the FASTA of hs_polish_haplotypes_from_files (the default parameters) in place of the bundle text; it wins over HS_CONSENSUS=1
    const char* want_hap = std::getenv("HS_HAPLOTYPES");
    if (want_hap && want_hap[0] == '1') {
        // HS_POLISH_PASSES=<n>: that many passes (hs_polish_haplotypes_refined); unset or 1: the one-pass call; anything else is refused there by name
        const char* passes = std::getenv("HS_POLISH_PASSES");
        if (passes && passes[0] && std::strcmp(passes, "1") != 0) {
            char* end = nullptr;
            const long n = std::strtol(passes, &end, 10);
            return hs_polish_haplotypes_refined_from_files(gfa, reads, sam, gro, polish_everything, nullptr, end && *end == 0 && n >= -1 && n <= 1000 ? (int32_t)n : -1, out_path, n_threads);
        }
        return hs_polish_haplotypes_from_files(gfa, reads, sam, gro, polish_everything, nullptr, out_path, n_threads);
    }
    try {
        hs::CvFileInput in;
        if (int rc = hs::load_cv_inputs(gfa, reads, sam, false, in, n_threads < 1 ? 1 : n_threads)) return rc;
        std::vector<std::vector<hs::LabelledInterval>> ivs;
        std::vector<uint8_t> has;
        if (int rc = hs::polish_intervals_from_gro(in, gro, ivs, has)) return rc;
        const int32_t n_contigs = (int32_t)in.contig_names.size();
        hs_cv_batch* b = nullptr;
        if (int rc = hs_cv_batch_create(in.contig_seq.data(), in.contig_off.data(), n_contigs, in.read_seq.data(), in.read_off.data(), (int32_t)in.read_names.size(),
                                        in.rec_read.data(), in.rec_pos.data(), in.rec_strand.data(), in.rec_cig_off.data(), in.cigar.data(), in.contig_rec_off.data(), &b))
            return rc;
        std::unique_ptr<hs_cv_batch, void (*)(hs_cv_batch*)> bguard(b, hs_cv_batch_destroy);
        hs_polish_result* r = nullptr;
        if (int rc = polish_inputs_core(b, 0, n_contigs, ivs, has, polish_everything != 0, &r)) return rc;
        std::unique_ptr<hs_polish_result, void (*)(hs_polish_result*)> rguard(r, hs_polish_result_destroy);
        // HS_CONSENSUS=1: every bundle's consensus (hs_polish_consensus, the default parameters) behind its text
        const char* want_cons = std::getenv("HS_CONSENSUS");
        hs_consensus_result* cons = nullptr;
        if (want_cons && want_cons[0] == '1') { if (int rc = hs_polish_consensus(r, nullptr, &cons)) return rc; }
        std::unique_ptr<hs_consensus_result, void (*)(hs_consensus_result*)> cguard(cons, hs_consensus_result_destroy);
        std::FILE* f = std::fopen(out_path, "wb");
        if (!f) { set_error(std::string("cannot write ") + out_path); return HS_EIO; }
        std::string text;
        bool ok = true;
        for (int64_t k = 0; k < r->n_bundles && ok; ++k) {
            text.clear();
            text += "BUNDLE\t" + in.contig_names[(size_t)r->bundle_contig[k]];
            const int32_t v[8] = {r->bundle_start[k], r->bundle_end[k], r->bundle_group[k], r->bundle_left_to_polish[k], r->bundle_right_to_polish[k],
                                  r->bundle_overhang_left[k], r->bundle_overhang_right[k], (int32_t)(r->piece_off[k + 1] - r->piece_off[k])};
            for (int32_t x : v) { text += '\t'; text += std::to_string(x); }
            text += "\n>seq\n";
            text.append((const char*)r->backbone + r->backbone_off[k], (size_t)(r->backbone_off[k + 1] - r->backbone_off[k]));
            text += '\n';
            for (int64_t p = r->piece_off[k]; p < r->piece_off[k + 1]; ++p) {
                if (r->base_off[p + 1] == r->base_off[p]) continue;      // tools.cpp:357
                text += ">read" + std::to_string(p - r->piece_off[k]) + " " + std::to_string(r->piece_sam_pos[p]) + " ";
                for (int64_t q = r->cig_off[p]; q < r->cig_off[p + 1]; ++q) { text += std::to_string(r->cigar[q] >> 4); text += "MIDNSHP=X???????"[r->cigar[q] & 15u]; }
                text += '\n';
                text.append((const char*)r->bases + r->base_off[p], (size_t)(r->base_off[p + 1] - r->base_off[p]));
                text += '\n';
            }
            if (cons) {
                text += ">consensus " + std::to_string(cons->trim_start[k]) + " " + std::to_string(cons->trim_end[k]) + "\n";
                text.append((const char*)cons->cons + cons->cons_off[k], (size_t)(cons->cons_off[k + 1] - cons->cons_off[k]));
                text += '\n';
            }
            ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
        }
        ok = std::fclose(f) == 0 && ok;
        if (!ok) { set_error(std::string("short write on ") + out_path); return HS_EIO; }
        return HS_OK;
    } catch (const std::exception& e) { set_error(std::string("hs_polish_inputs_from_files: ") + e.what()); return HS_EINVAL; }
}

// hs_polish_inputs <assembly.gfa> <reads> <aln.sam> <reads_haplo.gro> <polish_everything:0|1> <out> [threads]
int hs_polish_inputs_main(int argc, char** argv) {
    if (argc < 7) {
        std::printf("Usage: hs_polish_inputs <original_assembly.gfa> <reads_file> <sam_file> <gro_file> <polish_everything:0|1> <output> [num_threads]\n");
        return argc == 2 ? 0 : 1;
    }
    const int rc = hs_polish_inputs_from_files(argv[1], argv[2], argv[3], argv[4], std::atoi(argv[5]), argv[6], argc > 7 ? std::atoi(argv[7]) : 1);
    if (rc) std::printf("ERROR: %s\n", hs_last_error());
    return rc ? 1 : 0;
}
