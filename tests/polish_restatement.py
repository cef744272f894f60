"""The polisher's inputs of the reference's stage 5, restated per base in plain Python from the cited lines of
the reference's src/ (create_new_contigs.cpp unless another file is named). It walks the CIGAR expanded to one char per base, as
the reference does; the product (hs_kernels_polish.hip) walks the run-length ops. It is the oracle of the cut points, the
clipped CIGAR, startPosition and the dropped list, which the reference never writes out, and it reproduces the bytes the
reference does write (tests/golden/polish_inputs, test_cpu_polish_inputs.py).

Also here, because the goldens need them: the four input files read as the reference reads them (parse_reads, parse_assembly,
parse_SAM of input_output.cpp; parse_split_file :41-175) and merge_intervals with stitch (:1427-1534, :833-903)."""
import binascii
import hashlib

OPCHAR = "MIDNSHP=X"
START_BEYOND_SEQ = 2


# ---- tools.cpp:27-57 and :61-80 -------------------------------------------------------------------
def convert_cigar(cigar):
    if cigar == "*":
        return ""
    out, num = [], ""
    for c in cigar:
        if c.isdigit():
            num += c
        else:
            out.append(c * int(num))
            num = ""
    return "".join(out)


def convert_cigar2(expanded):
    res, number, current = "", 0, " "
    for c in expanded:
        if c == current or current == " ":
            number += 1
            current = c
        else:
            res += str(number) + current
            number, current = 1, c
    return res + str(number) + current


def cigar_words_to_string(words):
    return "".join("%d%s" % (int(w) >> 4, OPCHAR[int(w) & 15]) for w in words)


# ---- sequence.cpp:13-65 ---------------------------------------------------------------------------
def sequence_str(raw):
    """Sequence(raw).str(): anything but A C G is T (lower case included)"""
    return "".join(c if c in "ACG" else "T" for c in raw)


_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def reverse_complement(seq):
    return "".join(_COMPLEMENT[c] for c in reversed(seq))


def substr(s, pos, count):
    """std::string::substr(pos, (size_t)count): throws when pos > size, clamps the count, a negative int count is npos"""
    if pos > len(s):
        raise IndexError("substr")
    return s[pos:] if count < 0 else s[pos:pos + count]


# ---- :371-375, :517-519 ---------------------------------------------------------------------------
def bounds(L, start, end):
    overhang_left = min(start, 150)
    overhang_right = max(0, min(L - end - 1, 150))
    left = max(0, start - overhang_left)
    right = min(L - 1, end + overhang_right + 1)
    return overhang_left, overhang_right, left, right


def to_polish(backbone, start, end, overhang_left, overhang_right):
    L = len(backbone)
    return (substr(backbone, max(0, start - overhang_left), min(overhang_left, start)) + substr(backbone, start, end - start) +
            substr(backbone, end, min(overhang_right + 1, L - end - 1)))


# ---- :392-447 -------------------------------------------------------------------------------------
def walk(expanded, pos, left, right):
    """(posOnReadStart, posOnReadEnd, posOnCIGARStart, posOnCIGAREnd)"""
    on_read, on_cigar, on_interval = 0, 0, pos
    rs = re = cs = ce = -1
    for c in expanded:
        on_cigar += 1
        if c == "S" or c == "H":
            if rs != -1:
                re, ce = on_read, on_cigar - 1
                break
            on_read += 1
            continue
        if rs == -1 and on_interval >= left:
            rs, cs = on_read, on_cigar - 1
        if re == -1 and on_interval == right:
            re, ce = on_read, on_cigar - 1
            break
        if c == "M":
            on_read += 1
            on_interval += 1
        elif c == "D":
            on_interval += 1
        elif c == "I":
            on_read += 1
    if re == -1:
        re, ce = on_read, on_cigar
    return rs, re, cs, ce


def cut_read(read, strand, cigar, pos, left, right):
    """One read of one interval (:392-462). read: Sequence::str() of the read as sequenced. None when the read is dropped."""
    expanded = convert_cigar(cigar)
    rs, re, cs, ce = walk(expanded, pos, left, right)
    if rs > re or rs == -1:
        return None
    seq = read if strand else reverse_complement(read)
    flags = 0
    if rs > len(seq):
        flags, bases = START_BEYOND_SEQ, ""      # the reference's substr throws: the product flags the piece and leaves it empty
    else:
        bases = substr(seq, rs, re - rs)
    return {"read_start": rs, "read_end": re, "sam_pos": max(1, pos + 1 - left), "flags": flags, "bases": bases,
            "cigar": convert_cigar2(substr(expanded, cs, ce - cs)), "cigar_start": cs, "cigar_end": ce}


def contig_bundles(c, backbone, records, intervals, polish_everything, has_partitions=True):
    """The bundles of one contig (:358-521, :523) and the reads it drops. records: (read string, strand, pos, cigar string) per
    record of the contig; intervals: (start, end, labels) after merge_intervals. A bundle is one group of one interval; groups by
    ascending label (the reference iterates an unordered_map)."""
    L = len(backbone)
    if not has_partitions:
        if not polish_everything:
            return [], []
        intervals = [(0, L, [0] * len(records))]      # :249-251
    bundles, dropped = [], []
    for n, (start, end, labels) in enumerate(intervals):
        overhang_left, overhang_right, left, right = bounds(L, start, end)
        per_part, existing = {}, set()
        for r, lab in enumerate(labels):
            if lab > -1:
                existing.add(lab)
                read, strand, pos, cigar = records[r]
                piece = cut_read(read, strand, cigar, pos, left, right)
                if piece is None:
                    dropped.append((c, n, r))
                    continue
                piece["rec"] = r
                per_part.setdefault(lab, []).append(piece)
        clusters = sum(1 for k in per_part if k >= 0)
        if not per_part and len(labels) > 0 and not existing:
            per_part[-1] = []                          # :493-499
        for k in existing:
            per_part.setdefault(k, [])                 # :500-506
        if not (clusters > 1 or polish_everything):     # :523
            continue
        for group in sorted(per_part):
            bundles.append({"contig": c, "interval": n, "start": start, "end": end, "group": group, "left": left, "right": right,
                            "overhang_left": overhang_left, "overhang_right": overhang_right,
                            "to_polish": to_polish(backbone, start, end, overhang_left, overhang_right), "pieces": per_part[group]})
    return bundles, dropped


# ---- :833-903 and :1427-1534 ----------------------------------------------------------------------
def stitch(par, neighbor):
    fit_left, fit_right, size, st = {}, {}, {}, {}
    for a, b in zip(par, neighbor):
        if a > -1 and b > -1:
            fit_left.setdefault(a, {})
            fit_left[a][b] = fit_left[a].get(b, 0) + 1
            size[a] = size.get(a, 0) + 1
            st.setdefault(a, set())
            fit_right.setdefault(b, {})
            fit_right[b][a] = fit_right[b].get(a, 0) + 1
    for a, cands in fit_left.items():
        for b, n in cands.items():
            if n >= min(5.0, 0.7 * size[a]):
                st[a].add(b)
    for b, cands in fit_right.items():
        for a, n in cands.items():
            if n >= min(5.0, 0.7 * size[a]):
                st[a].add(b)
    return st


def merge_intervals(ivs):
    if not ivs:
        return []
    out = []
    (c_start, c_end, group) = ivs[0][0], ivs[0][1], list(ivs[0][2])
    for start, end, there in ivs[1:]:
        stitch_left = stitch(group, there)
        stitches = {k: set(v) for k, v in stitch_left.items()}
        left = set(group) - {-1, -2}
        right = set(there) - {-1, -2}
        stitched = set()
        for v in stitches.values():
            stitched |= v
        for cl in sorted(left):
            if cl not in stitched:
                for k in stitch_left:
                    stitches[k].add(cl)
        trivial, conversion, seen = True, {}, set()
        for k, v in stitches.items():
            if len(v) > 1:
                trivial = False
                continue
            only = next(iter(v)) if v else 0      # the reference dereferences begin() of an empty set: the value cannot matter
            if only in seen:
                trivial = False
            else:
                seen.add(only)
            conversion[only] = k
        if len(seen) < len(left) or len(left) != len(right):
            trivial = False
        if not trivial:
            out.append((c_start, c_end, group))
            group, c_start, c_end = list(there), start, end
        else:
            c_end = end
            for r in range(len(group)):
                if group[r] < 0 and there[r] > -1:
                    group[r] = conversion.get(there[r], 0)
    out.append((c_start, c_end, group))
    return out


# ---- the input files (input_output.cpp:39-536) -----------------------------------------------------
def parse_reads(path):
    """[(name, sequence line)] in file order; FASTA unless the name ends otherwise (:41-44)"""
    fasta = path.endswith(".fasta") or path.endswith(".fa")
    lines = open(path).read().split("\n")
    out = []
    if fasta:
        for i, l in enumerate(lines):
            if l.startswith(">"):
                out.append((l[1:].split(" ")[0], lines[i + 1]))
    else:
        for i in range(0, len(lines) - 3, 4):
            out.append((lines[i][1:].split(" ")[0], lines[i + 1]))
    return out


def parse_job(gfa, reads, sam):
    """contigs: [(name, sequence)] in GFA order; records[c]: [(read index, strand, pos, cigar)] in SAM order, as parse_SAM keeps them"""
    rd = parse_reads(reads)
    contigs = []
    for l in open(gfa):
        f = l.rstrip("\n").split("\t")
        if f[0] == "S":
            contigs.append((f[1].split(" ")[0], f[2]))
    index = {}
    for i, (nm, _) in enumerate(rd):
        index[nm] = i
    for i, (nm, _) in enumerate(contigs):
        index[nm] = len(rd) + i
    records = [[] for _ in contigs]
    for line in open(sam):
        line = line.rstrip("\n")
        if not line or line[0] == "@":
            continue
        f = line.split("\t")
        known = f[0] in index
        if not known:
            index[f[0]] = 0      # :317-325: the lookup of an unknown name inserts it with index 0; its NEXT line is a record of read 0
        if len(f) > 2 and f[2] not in index:
            index[f[2]] = 0      # :344
        if not known or len(f) <= 10:
            continue
        flag = int(f[1])
        if flag % 8 >= 4:
            continue
        seq1, seq2 = index[f[0]], index[f[2]]
        if seq1 == seq2:
            continue
        length1 = 0
        for t in f[6:]:
            if t.startswith("LN:i:"):
                length1 = int(t[5:])
        cigar = f[5]
        ops = []
        num = ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                ops.append((int(num), ch))
                num = ""
        hard = (ops[0][0] if ops and ops[0][1] == "H" else 0) + (ops[-1][0] if len(ops) > 0 and ops[-1][1] == "H" else 0)
        if hard > 0.2 * length1 and flag < 2048:
            continue
        if flag % 512 >= 256:
            continue
        if seq2 >= len(rd) and seq1 < len(rd):
            records[seq2 - len(rd)].append((seq1, flag % 32 < 16, int(f[3]) - 1, cigar))
    return rd, contigs, records


def parse_gro(path, rd, contigs, records):
    """partitions: {contig index: [(start, end, labels)]} (:41-175)"""
    cidx = {nm: i for i, (nm, _) in enumerate(contigs)}
    partitions, cur, names, neighbor = {}, None, [], {}
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "CONTIG":
            cur = cidx[t[1]]
            partitions[cur] = []
            names = []
            neighbor = {rd[r[0]][0]: n for n, r in enumerate(records[cur])}
        elif t[0] == "READ":
            names.append(t[1])
        elif t[0] == "GROUP":
            idx_s = t[3] if len(t) > 3 else ""
            lab_s = t[4] if len(t) > 4 else ""
            if idx_s == "," or lab_s == ",":
                continue
            idx = [int(x) for x in idx_s.split(",") if x != ""]
            lab = [int(x) for x in lab_s.split(",") if x != ""]
            full = [-2] * len(records[cur])
            for r, i in enumerate(idx):
                if names[i] in neighbor:
                    full[neighbor[names[i]]] = lab[r]
            partitions[cur].append((int(t[1]), int(t[2]), full))
    return partitions


def job_bundles(gfa, reads, sam, gro, polish_everything):
    """Every bundle of a job, contig by contig, and the dropped reads"""
    rd, contigs, records = parse_job(gfa, reads, sam)
    partitions = parse_gro(gro, rd, contigs, records)
    bundles, dropped = [], []
    strs = {}
    for c, (name, seq) in enumerate(contigs):
        recs = []
        for (r, strand, pos, cigar) in records[c]:
            if r not in strs:
                strs[r] = sequence_str(rd[r][1])
            recs.append((strs[r], strand, pos, cigar))
        b, d = contig_bundles(c, sequence_str(seq), recs, merge_intervals(partitions.get(c, [])), polish_everything, c in partitions)
        bundles += b
        dropped += d
    return bundles, dropped, [nm for nm, _ in contigs]


# ---- what the goldens record ------------------------------------------------------------------------
def bundle_key(to_polish_bytes, pieces):
    """pieces: [(k, bases)] of the non-empty pieces. The key a recorded bundle is compared by."""
    return (len(to_polish_bytes), hashlib.sha1(to_polish_bytes).hexdigest(),
            tuple((int(k), len(b), binascii.crc32(b) & 0xffffffff) for k, b in pieces))


def restated_keys(bundles):
    """sorted keys of the bundles that have at least one non-empty read (what the reference hands to its polisher)"""
    keys = []
    for b in bundles:
        pcs = [(k, p["bases"].encode()) for k, p in enumerate(b["pieces"]) if p["bases"]]
        if b["pieces"]:
            keys.append(bundle_key(b["to_polish"].encode(), pcs))
    return sorted(keys)


def parse_tool_output(path):
    """bin/hs_polish_inputs' text -> [{"head": fields of the BUNDLE line, "to_polish": str, "pieces": [(k, sam_pos, cigar, bases)]}]"""
    out = []
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        l = lines[i]
        if l.startswith("BUNDLE\t"):
            out.append({"head": l.split("\t")[1:], "to_polish": lines[i + 2], "pieces": []})
            i += 3
        elif l.startswith(">read"):
            k, sam_pos, cigar = l[5:].split(" ")
            out[-1]["pieces"].append((int(k), int(sam_pos), cigar, lines[i + 1]))
            i += 2
        else:
            i += 1
    return out
