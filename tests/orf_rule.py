"""The rule of mk_orf_* (include/mercat_hip.h) restated over Python bytes: what the tests compare Counter.orfs with.
Nothing here touches the library.

The text is read by the reference's line loop (as tests/trim_rule.records does): lines end at LF, CR LF or a lone CR; a
line whose stripped form starts with '>' opens a record; every other line gives ``line.strip().replace("*", "")`` to the
record it stands in -- to a leading record without a header line if none is open yet.

Six-frame stop-to-stop ORFs: for the record's kept characters and then their reverse complement, and each class c in
0, 1, 2, codon i covers t[c + 3i, c + 3i + 3).  A stretch is a maximal run of non-stop codons of one class; the ends of
the record close stretches too.  The reverse strand is done on a reverse-complemented copy and its coordinates turned
round afterwards: nothing here knows that both strands look alike from the forward one."""
import re

# index 16 c1 + 4 c2 + c3 with A 0, C 1, G 2, T 3
CODON_TABLE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
# NCBI translation table 1 as NCBI prints it: first base T C A G slowest, third base fastest
NCBI_TABLE_1 = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
STOPS = ("TAA", "TAG", "TGA")
START, ALT, PLUS, MINUS = 1, 2, 4, 8

_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)|[^\r\n]+")
_BLANKS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"  # what str.strip() removes from ASCII text
_CODE = {}
for _i, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _ch in _letters:
        _CODE[ord(_ch)] = _i


def records(text: bytes):
    """[(name -- b"" for the headless record --, kept characters)] in text order."""
    recs = []
    for line in _LINE.findall(bytes(text)):
        stripped = line.strip(_BLANKS)
        if stripped.startswith(b">"):
            name = bytearray()
            for b in stripped[1:]:
                if b <= 0x20:
                    break
                name.append(b)
            recs.append([bytes(name), b""])
        else:
            piece = stripped.replace(b"*", b"")
            if not recs and piece:
                recs.append([b"", b""])
            if recs:
                recs[-1][1] += piece
    return [(name, seq) for name, seq in recs]


def codes(seq: bytes):
    """0..3 per base, None for every other byte."""
    return [_CODE.get(b) for b in seq]


def revcomp(cs):
    return [None if c is None else 3 - c for c in reversed(cs)]


def translate(codon) -> str:
    if None in codon:
        return "X"
    return CODON_TABLE[16 * codon[0] + 4 * codon[1] + codon[2]]


def stretches(cs, c):
    """[(first codon index, end codon index, amino acids)] of class c of the coded string cs: maximal runs of non-stop
    codons, the empty ones included."""
    out, run, first = [], [], 0
    n = (len(cs) - c) // 3 if len(cs) >= c else 0
    for i in range(n):
        aa = translate(cs[c + 3 * i:c + 3 * i + 3])
        if aa == "*":
            out.append((first, i, "".join(run)))
            run, first = [], i + 1
        else:
            run.append(aa)
    out.append((first, n, "".join(run)))
    return out


def record_orfs(seq: bytes, min_aa: int = 32, flags: int = 0):
    """[(begin, aa, frame, amino acids)] of one record in the rule's order."""
    assert min_aa >= 1
    assert not (flags & ALT) or (flags & START)
    assert not ((flags & PLUS) and (flags & MINUS))
    L = len(seq)
    fwd = codes(seq)
    found = []  # (right end of the stretch, strand, begin, aa, frame, amino acids)
    starts = {14} | ({46, 62} if flags & ALT else set())  # ATG; GTG TTG
    for strand, cs in ((0, fwd), (1, revcomp(fwd))):
        if (strand == 0 and flags & MINUS) or (strand == 1 and flags & PLUS):
            continue
        for c in range(3):
            for first, end, aas in stretches(cs, c):
                a, b = c + 3 * first, c + 3 * end  # the stretch in the coordinates of cs
                right = b if strand == 0 else L - a
                if flags & START:
                    at = None
                    for i in range(first, end):
                        codon = cs[c + 3 * i:c + 3 * i + 3]
                        if None not in codon and 16 * codon[0] + 4 * codon[1] + codon[2] in starts:
                            at = i
                            break
                    if at is None:
                        continue
                    aas = aas[at - first:]
                    a = c + 3 * at
                if len(aas) < min_aa:
                    continue
                begin = a if strand == 0 else L - b
                found.append((right, strand, begin, len(aas), (1 if strand == 0 else 4) + c, aas))
    found.sort(key=lambda t: (t[0], t[1]))
    assert len({(t[0], t[1]) for t in found}) == len(found)
    return [t[2:] for t in found]


def expected(text: bytes, min_aa: int = 32, start: bool = False, alt_starts: bool = False, strand: str = "both"):
    """(output bytes, [[record, begin, aa, frame]]) of a whole text."""
    flags = (START if start else 0) | (ALT if alt_starts else 0) | {"both": 0, "plus": PLUS, "minus": MINUS}[strand]
    out, rows = [], []
    for r, (name, seq) in enumerate(records(text)):
        for n, (begin, aa, frame, aas) in enumerate(record_orfs(seq, min_aa, flags), 1):
            out.append(b">" + name + b"_%d_%d_%d\n" % (begin + 1, frame, n) + aas.encode() + b"\n")
            rows.append([r, begin, aa, frame])
    return b"".join(out), rows


def proteins(faa: bytes):
    """[(header text, sequence without a trailing '*')] of a protein FASTA."""
    out = []
    for block in faa.decode("latin-1").split(">")[1:]:
        head, _, body = block.partition("\n")
        out.append((head.strip(), "".join(body.split()).rstrip("*")))
    return out
