// hs_map_host.cpp -- the device-free half of the read mapper: the rule of hs_map_host.h over a whole job, on the host. It is the yardstick the
// device is held to by integer equality (tests/test_gpu_map.py through tests/harness/map_selftest.cpp) and the text of hs_map_text; the same for
// the split form (map_reads_split_host, hs_map_segments_text; tests/test_gpu_map_split.py through tests/harness/map_split_selftest.cpp). No HIP.
#include "hs_map_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

namespace hs {

void map_minimizers(const uint8_t* seq, const int64_t* off, int32_t n_seqs, const hs_map_params& p, MapMinimizers& out) {
    out.h.clear(); out.ps.clear(); out.seq.clear();
    out.seq_off.assign((size_t)n_seqs + 1, 0);
    std::vector<uint32_t> h, s;
    std::vector<uint8_t> ok, named;
    for (int32_t i = 0; i < n_seqs; ++i) {
        const int64_t L = off[i + 1] - off[i], n = L - p.k + 1;
        if (n >= 1) {
            h.assign((size_t)n, 0); s.assign((size_t)n, 0); ok.assign((size_t)n, 0); named.assign((size_t)n, 0);
            for (int64_t q = 0; q < n; ++q) ok[(size_t)q] = map_kmer(seq + off[i] + q, p.k, &h[(size_t)q], &s[(size_t)q]) ? 1 : 0;
            const int64_t last = map_last_window(n, p.w);
            for (int64_t j = 0; j <= last; ++j) {
                int64_t arg = -1;
                for (int64_t q = j; q < j + p.w && q < n; ++q)
                    if (ok[(size_t)q] && (arg < 0 || h[(size_t)q] < h[(size_t)arg])) arg = q;      // (strict: the leftmost of equal hashes stays)
                if (arg >= 0) named[(size_t)arg] = 1;
            }
            for (int64_t q = 0; q < n; ++q)
                if (named[(size_t)q]) { out.h.push_back(h[(size_t)q]); out.ps.push_back(((uint32_t)q << 1) | s[(size_t)q]); out.seq.push_back(i); }
        }
        out.seq_off[(size_t)i + 1] = (int64_t)out.h.size();
    }
}

int map_index_host(const uint8_t* contig_seq, const int64_t* contig_off, int32_t n_contigs, const hs_map_params& p, MapIndexHost& ix, std::string& err) {
    if (!map_params_valid(p) || n_contigs < 0 || !contig_off) { err = "map index: parameters out of range"; return HS_EINVAL; }
    ix.params = p; ix.n_contigs = n_contigs;
    ix.contig_len.resize((size_t)n_contigs);
    for (int32_t c = 0; c < n_contigs; ++c) {
        ix.contig_len[(size_t)c] = contig_off[c + 1] - contig_off[c];
        if (ix.contig_len[(size_t)c] < 0 || ix.contig_len[(size_t)c] > 0x7fffffff) { err = "map index: a contig of more than 2^31 bases"; return HS_EINVAL; }
    }
    MapMinimizers mz;
    map_minimizers(contig_seq, contig_off, n_contigs, p, mz);
    const size_t n = mz.h.size();
    ix.bucket_bits = map_bucket_bits(p, (int64_t)n);
    const uint32_t mask = (uint32_t)(((uint64_t)1 << ix.bucket_bits) - 1);
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {      // (stable: contig and t ascend inside equal (bucket, h))
        const uint32_t ba = mz.h[a] & mask, bb = mz.h[b] & mask;
        return ba != bb ? ba < bb : mz.h[a] < mz.h[b];
    });
    ix.bucket_off.assign(((size_t)1 << ix.bucket_bits) + 1, 0);
    ix.e_h.resize(n); ix.e_ts.resize(n); ix.e_c.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const size_t o = order[i];
        ix.e_h[i] = mz.h[o]; ix.e_ts[i] = mz.ps[o]; ix.e_c[i] = mz.seq[o];
        ix.bucket_off[(size_t)(mz.h[o] & mask) + 1]++;
    }
    for (size_t b = 0; b + 1 < ix.bucket_off.size(); ++b) ix.bucket_off[b + 1] += ix.bucket_off[b];
    return HS_OK;
}

namespace {
struct Hit { uint64_t key; int32_t qa, t; };

// the hits of one read (all of them, in minimizer order) and its minimizer counts
void map_read_hits(const MapIndexHost& ix, const uint8_t* seq, int64_t L, std::vector<Hit>& hits, int32_t* n_minimizers, int32_t* n_skipped) {
    const hs_map_params& p = ix.params;
    const int64_t off[2] = {0, L};
    MapMinimizers mz;
    map_minimizers(seq, off, 1, p, mz);
    const uint32_t mask = (uint32_t)(((uint64_t)1 << ix.bucket_bits) - 1);
    hits.clear();
    *n_skipped = 0;
    for (size_t m = 0; m < mz.h.size(); ++m) {
        const uint32_t h = mz.h[m];
        const int64_t b0 = ix.bucket_off[h & mask], b1 = ix.bucket_off[(size_t)(h & mask) + 1];
        int64_t occ = 0;
        for (int64_t e = b0; e < b1; ++e) occ += ix.e_h[(size_t)e] == h;
        if (occ > p.max_occ) { ++*n_skipped; continue; }
        for (int64_t e = b0; e < b1; ++e) {
            if (ix.e_h[(size_t)e] != h) continue;
            Hit x;
            x.t = (int32_t)(ix.e_ts[(size_t)e] >> 1);
            x.key = map_hit(ix.e_c[(size_t)e], x.t, ix.e_ts[(size_t)e] & 1u, (int32_t)(mz.ps[m] >> 1), mz.ps[m] & 1u, (int32_t)L, p, &x.qa);
            hits.push_back(x);
        }
    }
    *n_minimizers = (int32_t)mz.h.size();
}

// the vote over these keys (sorted here): best, its key, and second where asked for
void map_vote_keys(std::vector<uint64_t>& keys, bool want_second, MapVote& v) {
    std::sort(keys.begin(), keys.end());
    auto count = [&](uint64_t key) { auto rg = std::equal_range(keys.begin(), keys.end(), key); return (uint32_t)(rg.second - rg.first); };
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i && keys[i] == keys[i - 1]) continue;
        const uint32_t sc = count(keys[i]) + count(keys[i] + 1);
        if (v.best == 0 || map_beats(sc, keys[i], v.best, v.key)) { v.best = sc; v.key = keys[i]; }
    }
    for (size_t i = 0; want_second && i < keys.size(); ++i) {
        if ((i && keys[i] == keys[i - 1]) || !map_second_allowed(keys[i], v.key)) continue;
        v.second = std::max(v.second, count(keys[i]) + count(keys[i] + 1));
    }
}

void map_one_read(const MapIndexHost& ix, const uint8_t* seq, int64_t L, size_t r, MapResultHost& out, std::vector<Hit>& hits, std::vector<uint64_t>& keys, MapVote* vote = nullptr) {
    const hs_map_params& p = ix.params;
    map_read_hits(ix, seq, L, hits, &out.n_minimizers[r], &out.n_skipped[r]);
    keys.resize(hits.size());
    for (size_t i = 0; i < hits.size(); ++i) keys[i] = hits[i].key;
    MapVote v;
    map_vote_keys(keys, true, v);
    bool first = true;
    for (const Hit& x : hits) {
        if (!map_in_best(x.key, v.key)) continue;
        if (first) { v.qa_min = v.qa_max = x.qa; v.t_min = v.t_max = x.t; first = false; }
        v.qa_min = std::min(v.qa_min, x.qa); v.qa_max = std::max(v.qa_max, x.qa); v.t_min = std::min(v.t_min, x.t); v.t_max = std::max(v.t_max, x.t);
    }
    const int32_t Lc = v.best ? (int32_t)ix.contig_len[(size_t)map_key_contig(v.key)] : 0;
    map_interval(p, v, (int32_t)L, Lc, &out.contig[r], &out.strand[r], &out.qstart[r], &out.qend[r], &out.tstart[r], &out.tend[r]);
    out.votes[r] = (int32_t)v.best; out.second[r] = (int32_t)v.second;
    out.n_hits[r] = (int64_t)hits.size();
    if (vote) *vote = v;
}

// the anchors of one mapped read (hs_map_host.h, "anchors"): the best's hits as keys, then map_anchors_of_keys
struct ReadAnchors { std::vector<int32_t> q, t; int32_t n_best = 0, n_chain = 0, n_supported = 0; };
void map_anchors_one_read(const hs_map_anchor_params& ap, int64_t L, const std::vector<Hit>& hits, const MapVote& v, std::vector<uint64_t>& keys, ReadAnchors& a) {
    a = ReadAnchors();
    if (hits.size() > (size_t)HS_MAP_ANCHOR_CAPACITY) return;      // (the wide route: aligned the plain way)
    keys.clear();
    for (const Hit& x : hits)
        if (map_in_best(x.key, v.key)) keys.push_back(map_anchor_key(x.qa, x.t));
    a.n_best = (int32_t)keys.size();
    map_anchors_of_keys(ap, L, keys, a.q, a.t, &a.n_chain, &a.n_supported, nullptr);
}

// the split rule on one read: its sorted segments (n of them) and round 0's vote
int map_split_one_read(const MapIndexHost& ix, const hs_map_split_params& sp, int32_t Lr, const std::vector<Hit>& hits, std::vector<uint64_t>& keys, MapSegment* segs, MapVote& v0) {
    const hs_map_params& p = ix.params;
    int32_t a0[HS_MAP_MAX_SEGMENTS], a1[HS_MAP_MAX_SEGMENTS];
    int n = 0;
    for (int round = 0; round < sp.max_segments; ++round) {
        keys.clear();
        for (const Hit& x : hits)
            if (map_hit_free(a0, a1, n, map_hit_q(x.qa, map_key_rel(x.key), Lr, p.k), p.k)) keys.push_back(x.key);
        if (keys.empty()) break;
        MapVote v;
        map_vote_keys(keys, round == 0, v);
        if (round == 0) v0 = v;
        if (v.best < map_round_threshold(p, sp, round)) break;
        uint32_t cnt[HS_MAP_MAX_SEGMENTS + 1] = {0};
        for (const Hit& x : hits) {
            const int32_t q = map_hit_q(x.qa, map_key_rel(x.key), Lr, p.k);
            if (map_in_best(x.key, v.key) && map_hit_free(a0, a1, n, q, p.k)) cnt[map_hit_gap(a1, n, q)]++;
        }
        const int g = map_best_gap(cnt, n + 1);
        MapSegment s{};
        s.key = v.key; s.n = cnt[g]; s.second = v.second; s.round = round;
        bool first = true;
        for (const Hit& x : hits) {
            const int32_t q = map_hit_q(x.qa, map_key_rel(x.key), Lr, p.k);
            if (!map_in_best(x.key, v.key) || !map_hit_free(a0, a1, n, q, p.k) || map_hit_gap(a1, n, q) != g) continue;
            if (first) { s.qa_min = s.qa_max = x.qa; s.t_min = s.t_max = x.t; first = false; }
            s.qa_min = std::min(s.qa_min, x.qa); s.qa_max = std::max(s.qa_max, x.qa); s.t_min = std::min(s.t_min, x.t); s.t_max = std::max(s.t_max, x.t);
        }
        if (!map_segment_stands(sp, round, s.n, s.qa_min, (int64_t)s.qa_max + p.k)) break;
        map_seed_span(map_key_rel(s.key), Lr, s.qa_min, (int64_t)s.qa_max + p.k, &s.a0, &s.a1);
        a0[n] = s.a0; a1[n] = s.a1;
        segs[n++] = s;
    }
    map_segments_sort(segs, n);
    return n;
}
// what the three host jobs ask of their reads
int map_check_reads(const int64_t* read_off, int32_t n_reads, std::string& err) {
    if (n_reads < 0 || !read_off) { err = "map reads: bad arguments"; return HS_EINVAL; }
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] > 0x7fffffff) { err = "map reads: a read of more than 2^31 bases"; return HS_EINVAL; }
    return HS_OK;
}

// per_read(r, hits, keys) for every read of a job: the reads strided over the threads, each thread with its own scratch; one thread runs inline
template <class PerRead> void map_for_each_read(int32_t n_reads, int n_threads, PerRead per_read) {
    const size_t n = (size_t)n_reads;
    n_threads = std::max(1, std::min(n_threads, std::max(1, n_reads)));
    auto work = [&](int t) {
        std::vector<Hit> hits;
        std::vector<uint64_t> keys;
        for (size_t r = (size_t)t; r < n; r += (size_t)n_threads) per_read(r, hits, keys);
    };
    if (n_threads == 1) { work(0); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; ++t) th.emplace_back(work, t);
    for (std::thread& t : th) t.join();
}

void map_result_zero(MapResultHost& out, size_t n) {
    for (std::vector<int32_t>* v : {&out.contig, &out.qstart, &out.qend, &out.tstart, &out.tend, &out.votes, &out.second, &out.n_minimizers, &out.n_skipped}) v->assign(n, 0);
    out.strand.assign(n, 0); out.n_hits.assign(n, 0);
}
}  // namespace

int map_reads_host(const MapIndexHost& ix, const uint8_t* read_seq, const int64_t* read_off, int32_t n_reads, int n_threads, MapResultHost& out, std::string& err) {
    if (int rc = map_check_reads(read_off, n_reads, err)) return rc;
    map_result_zero(out, (size_t)n_reads);
    map_for_each_read(n_reads, n_threads, [&](size_t r, std::vector<Hit>& hits, std::vector<uint64_t>& keys) {
        map_one_read(ix, read_seq + read_off[r], read_off[r + 1] - read_off[r], r, out, hits, keys);
    });
    return HS_OK;
}

void map_anchors_of_keys(const hs_map_anchor_params& ap, int64_t Lr, std::vector<uint64_t>& keys, std::vector<int32_t>& q, std::vector<int32_t>& t, int32_t* n_chain,
                         int32_t* n_supported, std::vector<int32_t>* members) {
    std::sort(keys.begin(), keys.end());
    const int n = (int)keys.size();
    std::vector<uint16_t> chain((size_t)n + 1), pred((size_t)n + 1);
    bool rises = true;
    for (int i = 1; rises && i < n; ++i) rises = map_anchor_rises(keys.data(), i);
    int len = n;
    if (rises) for (int i = 0; i < n; ++i) chain[(size_t)i] = (uint16_t)i;
    else len = map_anchor_chain(keys.data(), n, chain.data(), pred.data());
    *n_chain = len; *n_supported = 0;
    for (int j = 0; j < len; ++j)      // (the supported members side by side, where the predecessor links were)
        if (map_anchor_supported(keys.data(), chain.data(), len, j)) pred[(size_t)(*n_supported)++] = chain[(size_t)j];
    if (members) { members->clear(); for (int j = 0; j < len; ++j) members->push_back((int32_t)chain[(size_t)j]); }
    const int64_t cap = map_anchor_bound(Lr, ap.spacing);
    q.assign((size_t)cap, 0); t.assign((size_t)cap, 0);
    const int m = map_anchor_cuts(keys.data(), pred.data(), *n_supported, ap.spacing, q.data(), t.data(), cap);
    q.resize((size_t)m); t.resize((size_t)m);
}

int map_anchors_host(const MapIndexHost& ix, const hs_map_anchor_params& ap, const uint8_t* read_seq, const int64_t* read_off, int32_t n_reads, int n_threads, MapResultHost& out,
                     MapAnchorsHost& anchors, std::string& err) {
    if (!map_anchor_params_valid(ap)) { err = "map reads: anchor parameters out of range (spacing >= 1)"; return HS_EINVAL; }
    if (int rc = map_check_reads(read_off, n_reads, err)) return rc;
    const size_t n = (size_t)n_reads;
    map_result_zero(out, n);
    std::vector<ReadAnchors> per(n);
    map_for_each_read(n_reads, n_threads, [&](size_t r, std::vector<Hit>& hits, std::vector<uint64_t>& keys) {
        MapVote v;
        const int64_t L = read_off[r + 1] - read_off[r];
        map_one_read(ix, read_seq + read_off[r], L, r, out, hits, keys, &v);
        if (out.contig[r] >= 0) map_anchors_one_read(ap, L, hits, v, keys, per[r]);
    });
    anchors.anc_off.assign(n + 1, 0);
    anchors.anc_q.clear(); anchors.anc_t.clear();
    anchors.n_best.assign(n, 0); anchors.n_chain.assign(n, 0); anchors.n_supported.assign(n, 0);
    for (size_t r = 0; r < n; ++r) {
        anchors.anc_q.insert(anchors.anc_q.end(), per[r].q.begin(), per[r].q.end());
        anchors.anc_t.insert(anchors.anc_t.end(), per[r].t.begin(), per[r].t.end());
        anchors.anc_off[r + 1] = (int64_t)anchors.anc_q.size();
        anchors.n_best[r] = per[r].n_best; anchors.n_chain[r] = per[r].n_chain; anchors.n_supported[r] = per[r].n_supported;
    }
    return HS_OK;
}

int map_reads_split_host(const MapIndexHost& ix, const hs_map_split_params& sp, const uint8_t* read_seq, const int64_t* read_off, int32_t n_reads, int n_threads, MapSegmentsHost& out,
                         std::string& err) {
    if (!map_split_params_valid(sp)) { err = "map reads: split parameters out of range"; return HS_EINVAL; }
    if (int rc = map_check_reads(read_off, n_reads, err)) return rc;
    const size_t n = (size_t)n_reads;
    for (std::vector<int32_t>* v : {&out.n_minimizers, &out.n_skipped, &out.read_votes, &out.read_second}) v->assign(n, 0);
    out.n_hits.assign(n, 0);
    std::vector<MapSegment> segs(n * HS_MAP_MAX_SEGMENTS);
    std::vector<int32_t> n_segs(n, 0);
    map_for_each_read(n_reads, n_threads, [&](size_t r, std::vector<Hit>& hits, std::vector<uint64_t>& keys) {
        const int32_t Lr = (int32_t)(read_off[r + 1] - read_off[r]);
        map_read_hits(ix, read_seq + read_off[r], Lr, hits, &out.n_minimizers[r], &out.n_skipped[r]);
        out.n_hits[r] = (int64_t)hits.size();
        MapVote v0;
        n_segs[r] = map_split_one_read(ix, sp, Lr, hits, keys, &segs[r * HS_MAP_MAX_SEGMENTS], v0);
        out.read_votes[r] = (int32_t)v0.best; out.read_second[r] = (int32_t)v0.second;
    });
    out.seg_off.assign(n + 1, 0);
    for (size_t r = 0; r < n; ++r) out.seg_off[r + 1] = out.seg_off[r] + n_segs[r];
    const size_t S = (size_t)out.seg_off[n];
    for (std::vector<int32_t>* v : {&out.read, &out.contig, &out.qstart, &out.qend, &out.tstart, &out.tend, &out.votes, &out.second, &out.round}) v->assign(S, 0);
    out.strand.assign(S, 0);
    for (size_t r = 0; r < n; ++r) {
        const MapSegment* s = &segs[r * HS_MAP_MAX_SEGMENTS];
        const int32_t Lr = (int32_t)(read_off[r + 1] - read_off[r]);
        for (int i = 0; i < n_segs[r]; ++i) {
            const size_t o = (size_t)out.seg_off[r] + (size_t)i;
            const int32_t Lc = (int32_t)ix.contig_len[(size_t)map_key_contig(s[i].key)];
            map_segment_interval(ix.params, sp, s, n_segs[r], i, Lr, Lc, &out.contig[o], &out.strand[o], &out.qstart[o], &out.qend[o], &out.tstart[o], &out.tend[o]);
            out.read[o] = (int32_t)r; out.votes[o] = (int32_t)s[i].n; out.second[o] = (int32_t)s[i].second; out.round[o] = s[i].round;
        }
    }
    return HS_OK;
}

namespace {
void paf_columns(std::string& s, const std::string& read, int64_t read_len, int32_t qstart, int32_t qend, uint8_t strand, const std::string& contig, int64_t contig_len, int32_t tstart,
                 int32_t tend, int32_t votes, int32_t second) {
    s += read;
    s += '\t'; s += std::to_string(read_len);
    s += '\t'; s += std::to_string(qstart);
    s += '\t'; s += std::to_string(qend);
    s += strand ? "\t+\t" : "\t-\t";
    s += contig;
    s += '\t'; s += std::to_string(contig_len);
    s += '\t'; s += std::to_string(tstart);
    s += '\t'; s += std::to_string(tend);
    s += '\t'; s += std::to_string(votes);
    s += '\t'; s += std::to_string(tend - tstart);
    s += "\t255\ts1:i:"; s += std::to_string(votes);
    s += "\ts2:i:"; s += std::to_string(second);
}
}  // namespace

std::string map_segments_text(const hs_map_segments* r, const char* const* read_names, const int64_t* read_len, const char* const* contig_names, const int64_t* contig_len) {
    std::string s;
    for (int32_t i = 0; i < r->n_reads; ++i)
        for (int64_t j = r->seg_off[i]; j < r->seg_off[i + 1]; ++j) {
            const int32_t c = r->contig[j];
            paf_columns(s, read_names && read_names[i] ? std::string(read_names[i]) : "r" + std::to_string(i), read_len[i], r->qstart[j], r->qend[j], r->strand[j],
                        contig_names && contig_names[c] ? std::string(contig_names[c]) : "c" + std::to_string(c), contig_len[c], r->tstart[j], r->tend[j], r->votes[j], r->second[j]);
            s += "\tsg:i:"; s += std::to_string(r->round[j]);
            s += "\tns:i:"; s += std::to_string(r->seg_off[i + 1] - r->seg_off[i]);
            s += '\n';
        }
    return s;
}

std::string map_text(const hs_map_result* r, const char* const* read_names, const int64_t* read_len, const char* const* contig_names, const int64_t* contig_len) {
    std::string s;
    for (int32_t i = 0; i < r->n_reads; ++i) {
        const int32_t c = r->contig[i];
        if (c < 0) continue;
        paf_columns(s, read_names && read_names[i] ? std::string(read_names[i]) : "r" + std::to_string(i), read_len[i], r->qstart[i], r->qend[i], r->strand[i],
                    contig_names && contig_names[c] ? std::string(contig_names[c]) : "c" + std::to_string(c), contig_len[c], r->tstart[i], r->tend[i], r->votes[i], r->second[i]);
        s += '\n';
    }
    return s;
}

}  // namespace hs

namespace {
// the body of the two text entries: the lengths from the offsets, the lines, a malloc'd copy for the caller (hs_free_host)
template <class Lines> int map_text_copy(int32_t n_reads, const int64_t* h_read_off, int32_t n_contigs, const int64_t* h_contig_off, char** text, Lines lines) {
    std::vector<int64_t> rl((size_t)n_reads), cl((size_t)n_contigs);
    for (int32_t i = 0; i < n_reads; ++i) rl[(size_t)i] = h_read_off[i + 1] - h_read_off[i];
    for (int32_t c = 0; c < n_contigs; ++c) cl[(size_t)c] = h_contig_off[c + 1] - h_contig_off[c];
    const std::string s = lines(rl.data(), cl.data());
    *text = (char*)std::malloc(s.size() + 1);
    if (!*text) return HS_EINVAL;
    std::memcpy(*text, s.c_str(), s.size() + 1);
    return HS_OK;
}
}  // namespace

extern "C" {

hs_map_params hs_map_params_default(void) {
    hs_map_params p;
    p.k = 15; p.w = 10; p.max_occ = 64; p.band_log2 = 9; p.min_votes = 3; p.extend = 1; p.bucket_bits = -1;
    return p;
}
hs_map_anchor_params hs_map_anchor_params_default(void) {
    hs_map_anchor_params a;
    a.spacing = 256;      // (the fastest of one sweep on one job; not tuned beyond that)
    return a;
}
void hs_map_anchors_destroy(hs_map_anchors* a) {
    if (!a) return;
    void* p[] = {a->anc_off, a->anc_q, a->anc_t, a->n_best, a->n_chain, a->n_supported};
    for (void* q : p) std::free(q);
    std::free(a);
}
hs_map_split_params hs_map_split_params_default(void) {
    hs_map_split_params s;
    s.max_segments = 4; s.min_votes = 3; s.min_span = 100; s.max_gap = 200;      // (placeholders, not tuned)
    return s;
}
void hs_map_segments_destroy(hs_map_segments* r) {
    if (!r) return;
    void* p[] = {r->seg_off, r->read, r->contig, r->strand, r->qstart, r->qend, r->tstart, r->tend, r->votes, r->second, r->round, r->n_minimizers, r->n_skipped, r->n_hits,
                 r->read_votes, r->read_second};
    for (void* q : p) std::free(q);
    std::free(r);
}
int hs_map_segments_text(const hs_map_segments* segments, const char* const* read_names, const int64_t* h_read_off, const char* const* contig_names, const int64_t* h_contig_off,
                         int32_t n_contigs, char** text) {
    if (!segments || !h_read_off || !h_contig_off || !text || n_contigs < 0 || !segments->seg_off || segments->n_reads < 0 || segments->n_segments < 0) return HS_EINVAL;
    if (segments->seg_off[0] != 0 || segments->seg_off[segments->n_reads] != segments->n_segments) return HS_EINVAL;      // (the offsets say where the text reads)
    for (int32_t i = 0; i < segments->n_reads; ++i)
        if (segments->seg_off[i + 1] < segments->seg_off[i]) return HS_EINVAL;
    for (int64_t j = 0; j < segments->n_segments; ++j)
        if (segments->contig[j] < 0 || segments->contig[j] >= n_contigs) return HS_EINVAL;
    return map_text_copy(segments->n_reads, h_read_off, n_contigs, h_contig_off, text,
                         [&](const int64_t* rl, const int64_t* cl) { return hs::map_segments_text(segments, read_names, rl, contig_names, cl); });
}
void hs_map_result_destroy(hs_map_result* r) {
    if (!r) return;
    void* p[] = {r->contig, r->strand, r->qstart, r->qend, r->tstart, r->tend, r->votes, r->second, r->n_minimizers, r->n_skipped, r->n_hits};
    for (void* q : p) std::free(q);
    std::free(r);
}
int hs_map_text(const hs_map_result* result, const char* const* read_names, const int64_t* h_read_off, const char* const* contig_names, const int64_t* h_contig_off,
                int32_t n_contigs, char** text) {
    if (!result || !h_read_off || !h_contig_off || !text || n_contigs < 0) return HS_EINVAL;
    for (int32_t i = 0; i < result->n_reads; ++i)
        if (result->contig[i] >= n_contigs) return HS_EINVAL;
    return map_text_copy(result->n_reads, h_read_off, n_contigs, h_contig_off, text,
                         [&](const int64_t* rl, const int64_t* cl) { return hs::map_text(result, read_names, rl, contig_names, cl); });
}

}  // extern "C"
