"""Planted libraries and queries for tier 1's running top-L (ngs_kernels.hip: wave_flush, wave_sort64,
wave_trim, wave_select, term_pairs' w_max prune, raised_cmin's tie rule, emit_rank_prefix's key set and
k_merge's join), and the CPU facts about them. tests/test_topl_cases.py proves every claim on the CPU;
tests/test_gpu_topl_planted.py runs the libraries on the device, exact against the oracle, with the
route asserted from ngsLastStats.

The family trick. A family f has a 5-character prefix P_f over the digits and . % $ @ whose three grams
occur nowhere else in its library, n_f target terms P_f + a suffix over N..T, and the query
Q_f = P_f + "UVWXYZU" (12 characters, 10 grams; no row holds one of the tail's grams). Every target
shares exactly the prefix's 3 grams with Q_f, so its match ratio is s = fl(3 / 10), which passes
threshold 0.3 (s < thr is false at equality) and 0.2; nothing else scores 2 hits or more. Q_f therefore
has exactly one record per (target, key) pair, of score fl(w * s) for the pair's weight w, and its key
rank follows from key length and row order. Words are 9 characters unless said otherwise, so a key's
rank is its row's position among the rows.

Spread and dense. The main launch counts a part's candidates in a sketch and hands the query to tier 1b
when a part has more than 64 candidate entries (count()'s nc <= 64): a target is in three lists, so it
is 3 entries. A part holds at most 3 * 22 sixteen-byte chunks of one list (264 postings; half of that at
cmin 2). A "spread" family of more than 21 targets follows every target with 12 fillers per prefix gram
(a filler holds that one gram once: 1 hit, below cmin 2), so each of its three lists has 13 postings per
target and a part has at most 21 targets, 63 entries. A "dense" family's targets have consecutive term
ids (192 or more of them), so some part has more than 64 entries.
A "split" family has its first half at the head of the library and its second half at its end (the
first and the last skip bucket): parts ascend by bucket, so the halves arrive in different refills, and
in different slices ahead of k_merge.

Libraries (none above 40,000 rows, no family above 600 targets):
  n1..n3  spread, family N: 14 record counts around the buffer's 64-record batches and 256 records; in
     n3 also P (promotion among scores around 100; its query is a row, and fillers hold its tail grams too);
  o1..o3  spread, family O (600 scores descending, ascending, best in the last bucket); in o1 also T2 (a
     tie at tau whose later record has the better key rank; its weight is the library's largest), in o2
     and o3 B1 and B2 (the select's boundary bins);
  e1, e2  spread, families E (equal scores: a..e), B3 and T (400 records at the bound fl(w_max * s)),
     every word of one length (tk_monotone on); Ea's and T's weight is the library's largest, so their
     bound ties tau's score;
  d  dense versions of N (192 and more), O, Ec and B;
  u  small lists (at most 135 postings: 8 skip buckets, so the latency path's tier 1b stays unsliced):
     N up to 129, Ea, family M (two alias words under 300 keys each, weights ascending and descending
     over the pairs, beside 60 ordinary targets), and Uo and Ut (lib_u), whose 600 and 390 records come
     from 5 and 3 keys per word;
  a  rows of a key and two aliases, family A1 (both aliases in the key's row) and A2 (the aliases in
     two rows of the key, at the head and the end of the library), 400 keys each, fast_cases.D_WEIGHTS,
     and family M with fillers;
  r  one weight, threshold 0: the rank lists (emit_rank_prefix).
"""
import os
import random
import re
import struct

import numpy as np

import build_ref
from fast_cases import D_WEIGHTS, grams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_H = os.path.join(ROOT, "stringsearchlib_amd", "csrc", "ngs_common.h")


def read_geometry(text=None):
    if text is None:
        with open(COMMON_H) as f:
            text = f.read()
    out = {}
    for name in ("kWaveCand", "kWaveMaxLimit", "kMaxBuckets", "kMinBucketTerms", "kDenseBucketLen", "kHeavyCmin"):
        m = re.search(rf"constexpr \w+ {name} = (\d+);", text)
        if not m:
            raise RuntimeError(f"topl_cases: {name} not found in {COMMON_H}: tier 1's geometry moved, so the planted "
                               f"inputs of tests/topl_cases.py must be looked at again")
        out[name] = int(m.group(1))
    return out


GEOM = read_geometry()
CAND, MAX_LIMIT = GEOM["kWaveCand"], GEOM["kWaveMaxLimit"]
if CAND != 256 or MAX_LIMIT != 128 or GEOM["kHeavyCmin"] != 2:
    raise RuntimeError("topl_cases: the planted record counts and limits are for a buffer of 256 records, limits up "
                       "to 128 and a heavy list at cmin 2")

PLANT = "0123456789.%$@"
AM = "ABCDEFGHIJKLM"
SUF = "NOPQRST"
TAIL, TAIL_P = "UVWXYZU", "UZYXWVU"   # the queries' tails (family P's own: its query is a row)
FAR = "VW"                             # the flag twins' far rows
PART_POSTINGS = 4 * 3 * 22             # what a main-launch part can hold of one list: 3 G chunks, G <= 22 lanes
PART_TARGETS = 21                      # 3 candidate entries per target: 63 of the 64 a part may have
FILL = 12                              # fillers per target and prefix gram in a spread family
LIMITS = (1, 2, 63, 64, 65, 127, 128)


def f32(x):
    return np.float32(x)


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def from_bits(b):
    return f32(struct.unpack("<f", struct.pack("<I", b))[0])


S3 = f32(3) / f32(10)
assert bits(S3) == bits(f32(0.3)) and not S3 < f32(0.3)  # 3 hits of 10 pass threshold 0.3


def score_bits(w, s=S3):
    """calcScore's std::max(w * s, 0.0f) in fp32."""
    v = f32(w) * s
    return bits(v) if v > 0 else 0


def weight_for(vbits, s=S3):
    """A weight w with fl(w * s) == the fp32 value of bits vbits (values in [0.5, 0.6): there a step of
    w moves the product by 0.6 ulp, so every value is reached)."""
    v = from_bits(vbits)
    w0 = bits(f32(float(v) / float(s)))
    for d in range(0, 9):
        for wb in (w0 + d, w0 - d):
            if score_bits(from_bits(wb), s) == vbits:
                return float(from_bits(wb))
    raise AssertionError(f"no weight gives {vbits:#x}")


def enc_of(sbits):
    return sbits + 1 if sbits else 1


def record(sbits, rank):
    """The 64-bit buffer record: smaller is better (ScoreComparer: score descending, key rank ascending)."""
    return ((~enc_of(sbits) & 0xFFFFFFFF) << 32) | rank


def skip_buckets(n_long, max_len):
    """ngs_common.h's skip_buckets (the byte budget apart, which these libraries are far below)."""
    K = 1
    while K < GEOM["kMaxBuckets"] and K * GEOM["kMinBucketTerms"] < n_long:
        K <<= 1
    while K * 2 <= n_long and max_len // K > GEOM["kDenseBucketLen"]:
        K <<= 1
    return K, (n_long + K - 1) // K if n_long else 1


def _digits(i, alphabet, n):
    out = []
    for _ in range(n):
        out.append(alphabet[i % len(alphabet)])
        i //= len(alphabet)
    assert i == 0
    return "".join(reversed(out))


# ---- wave_select's digit choice, restated (proves which branches a record set reaches; NOT the reference) ----
def select_trace(records, L):
    """The passes of wave_select(records, L): per pass the digit's shift, the boundary bin b (lane b // 4,
    j = b % 4), and whether the L-th record is the last (k == incl) or the first (k == excl + 1) of its
    bin. Returns (passes, kth)."""
    assert 1 <= L <= len(records) <= CAND and len(set(records)) == len(records)
    pre = pm = 0
    k = L
    passes = []
    while True:
        match = [r for r in records if r & pm == pre]
        o = a = match[0]
        for r in match:
            o |= r
            a &= r
        d = o ^ a
        if not d:
            return passes, o
        top = d.bit_length() - 1
        sh = top - 7 if top >= 7 else 0
        above = 0 if top == 63 else ~((2 << top) - 1) & (2**64 - 1)
        hist = [0] * 256
        for r in match:
            hist[(r >> sh) & 255] += 1
        excl = 0
        for b in range(256):
            if excl < k <= excl + hist[b]:
                break
            excl += hist[b]
        passes.append({"sh": sh, "top": top, "bin": b, "lane": b // 4, "j": b % 4, "last": k == excl + hist[b],
                       "first": k == excl + 1, "in_bin": hist[b]})
        k -= excl
        pre = (o & above) | (b << sh)
        pm = above | (0xFF << sh)


# ---- families ------------------------------------------------------------------------------------
class Family:
    """weights: one per target in term-id order. lengths: the targets' lengths (9 unless given)."""

    def __init__(self, name, weights, spread=True, split=False, lengths=None, tail=TAIL):
        self.name, self.weights, self.split, self.tail = name, [float(f32(w)) for w in weights], split, tail
        self.n = len(weights)
        self.fill = spread and self.n > PART_TARGETS
        self.lengths = lengths or [9] * self.n
        self.prefix = self.query = None
        self.targets = []   # the words, in term-id order

    def scores(self):
        return [score_bits(w) for w in self.weights]


def _shuffled(values, seed):
    v = list(values)
    random.Random(seed).shuffle(v)
    return v


W_MAX = 1.984375  # the largest weight of libraries e and u (family Ea carries it)
N_SIZES = (1, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 320, 600)
V0 = bits(f32(0.55)) | 0xFFFF   # enc = V0 + 1: its low 16 bits are 0, so ~enc's are all ones ...
V_TOP = (bits(f32(0.55)) | 0xFFFF) - 1  # ... and here enc's low byte is 0xFF: ~enc's is 0, the first bin


def family_n(n, **kw):
    """n distinct scores in a shuffled order of arrival."""
    return Family(f"N{n}", _shuffled([1.0 + i / 1024 for i in range(n)], n), **kw)


def families_o(**kw):
    desc = Family("Odesc", [1.6 - i / 1024 for i in range(600)], **kw)
    asc = Family("Oasc", [1.0 + i / 1024 for i in range(600)], **kw)
    last = Family("Olast", _shuffled([1.0 + i / 1024 for i in range(300)], 3)
                  + _shuffled([1.5 + i / 1024 for i in range(300)], 4), split=True, **kw)
    return [desc, asc, last]


def family_ea():
    """21 records (no fillers between them) of one score (the library's largest weight: the bound fl(w_max * s) ties tau) at key ranks
    inside one aligned block of 128: after the score bits the records differ only below bit 7."""
    return Family("Ea", [W_MAX] * 21)


def family_eb():
    """200 records of one score, 100 at the head and 100 at the end of the library."""
    return Family("Eb", [1.25] * 200, split=True)


EC_RUNS = ((1.4, 50), (1.5, 100), (1.3, 50), (1.2, 400))


def family_ec(**kw):
    """Runs of equal scores; by score: 100, then 50, 50, 400. The limits 1, 100 / 101, 150 / 151 are the
    first and last records of runs, 2, 63..65, 127 and 128 inner ones."""
    return Family("Ec", [w for w, k in EC_RUNS for _ in range(k)], **kw)


def family_ed():
    """150 scores one ulp apart, shuffled."""
    return Family("Ed", _shuffled([weight_for(V0 - 7 - i) for i in range(150)], 5))


def family_ee():
    """Scores over 80 exponents, and +0 twenty times (negative weights), shuffled."""
    return Family("Ee", _shuffled([2.0 ** k for k in range(-80, 0)] + [-(2.0 ** k) for k in range(-10, 10)], 6))


def families_b(**kw):
    """B1: 256 scores one ulp apart whose best is in bin 0: every bin holds one record, so the L-th is the
    first and the last of its bin, at lane 0 (j = 0..3) for limits 1..4; one pass.
    B2: 60 scores one ulp apart (bins 0..59), then 35 records at each of the 4 scores in bins 252..255:
    limits above 60 end in lane 63, and go on by key rank.
    B3: 128 records, two keys at each of 64 scores that differ in bits 16..17, 8..9 and 0..1 of the score:
    the digit moves down the score and then to the key rank, 4 passes or more."""
    b1 = Family("B1", _shuffled([weight_for(V_TOP - i) for i in range(256)], 7), **kw)
    b2 = Family("B2", _shuffled([weight_for(V_TOP - i) for i in range(60)]
                                + [weight_for(V_TOP - i) for i in range(252, 256) for _ in range(35)], 8), **kw)
    b3 = Family("B3", _shuffled([weight_for(V_TOP - (a << 16 | b << 8 | c)) for a in range(4) for b in range(4)
                                 for c in range(4) for _ in range(2)], 9), **kw)
    return [b1, b2, b3]


def family_p():
    """The query is a key itself (promoted to 100); 42 keys score around 100: the weights are the 7 floats
    around 100 / s, whose products with s lie below and above 100 (and at it where fp32 allows), six keys
    each, then some far below and above."""
    w0 = bits(f32(100.0 / float(S3)))
    ws = [float(from_bits(w0 + d)) for d in range(-3, 4)]
    return Family("P", _shuffled(ws * 6 + [1.0, 2.0, 300.0, 340.0], 10), tail=TAIL_P)


O_WMAX = 2.0  # the largest weight of library o: family T2 carries it


def family_t2():
    """400 records of one score, fl(w_max * s) of their library: after the first refill (at 256) every later term's
    bound ties tau's score. The last target is one character shorter, so it arrives last and has the best
    key rank of all: a tie at tau that term_pairs must keep (ub_enc < te is false) and that wins."""
    return Family("T2", [O_WMAX] * 400, lengths=[9] * 399 + [8])


def family_t():
    """400 records of the score fl(w_max * s) in a library whose term ids ascend with the key ranks: the
    later records tie tau's score and lose on the rank (raised_cmin may drop their count under tk_monotone)."""
    return Family("T", [W_MAX] * 400)


# ---- libraries -------------------------------------------------------------------------------------
class Lib:
    """rows / weights as the index takes them (row_size words per row, None for a missing alias)."""

    def __init__(self, name, families, row_size=1, dense=False, seed=1):
        self.name, self.families, self.row_size, self.dense = name, list(families), row_size, dense
        self.rng = random.Random(seed)
        self.used = set()      # prefix grams
        self.seen = set()      # fillers' letters
        self.last = set()      # prefixes' last characters
        self.words, self.weights = [], []
        self.far = []          # (words of one row, weights) appended by twin()
        for f in self.families:
            self._name(f)

    # -- words
    def _name(self, f):
        while True:
            p = "".join(self.rng.choices(PLANT, k=5))
            g = set(grams(p))
            # (a last character of its own while there are some left: the gram P4 + "NN" of the first 49
            # suffixes then stays one family's)
            if len(g) == 3 and not g & self.used and (p[4] not in self.last or len(self.last) >= len(PLANT)):
                break
        self.used |= g
        self.last.add(p[4])
        f.prefix, f.query = p, p + f.tail
        f.targets = [p + _digits(i % len(SUF) ** (ln - 5), SUF, ln - 5) for i, ln in enumerate(f.lengths)]
        assert len(set(f.targets)) == f.n

    def filler(self, gram=None):
        """A 9-letter word over A..M, with `gram` in its middle."""
        while True:
            d = "".join(self.rng.choices(AM, k=6 if gram else 9))
            if d not in self.seen:
                break
        self.seen.add(d)
        return d[:3] + gram + d[3:] if gram else d

    def row(self, words, weights):
        words, weights = list(words), list(weights)
        while len(words) < self.row_size:
            words.append(None)
            weights.append(1.0)
        assert len(words) == self.row_size
        self.words += words
        self.weights += weights

    def fillers_of(self, f, k=1):
        """The fillers that follow k targets of a spread family, as single words."""
        return [self.filler(g) for _ in range(k) for g in grams(f.prefix) for _ in range(FILL)] if f.fill else []

    def finish(self):
        self.n_rows = len(self.words) // self.row_size
        # (family A: 400 keys as its dedup needs, so 800 alias targets)
        assert self.n_rows <= 40000 and all(f.n <= (800 if f.name[0] == "A" else 600) for f in self.families), self.name
        live = [w for w in self.words if w is not None]
        assert len(set(live)) == len(live) or self.name[0] in "uam" or "+" in self.name, self.name
        return self

    def encoded(self):
        return [None if w is None else w.encode() for w in self.words]

    def model(self):
        if not hasattr(self, "_model"):
            self._model = build_ref.build(self.encoded(), self.row_size, self.weights)
            assert self._model.n_short == 0
        return self._model


def single_lib(name, families, row_size=1, dense=False, seed=1, pad_to=None):
    """One word per row. Split families' first halves, the other families, (padding,) the second halves. A
    family whose query has its own tail (P) gets the query itself as a row behind its targets."""
    lib = Lib(name, families, row_size, dense, seed)

    def put(f, lo, hi):
        for i in range(lo, hi):
            lib.row([f.targets[i]], [f.weights[i]])
            for w in lib.fillers_of(f):
                lib.row([w], [1.0])

    for f in lib.families:
        if f.split:
            put(f, 0, f.n // 2)
    for f in lib.families:
        if not f.split:
            while f.name == "Ea" and len(lib.words) // row_size % 128:  # its key ranks in one aligned block of 128
                lib.row([lib.filler()], [1.0])
            put(f, 0, f.n)
            if f.tail != TAIL:
                for w in lib.fillers_of(f, 10):  # (its 10 entries in a part of few targets)
                    lib.row([w], [1.0])
                lib.row([f.query], [1.0])  # the exact match
                # other holders for the 7 grams behind the prefix: as the only row with them, the query's row
                # would end seven one-posting lists that lie side by side in the posting array, the sketch
                # would add each list's chunk neighbours (the same term) to one cell, and the cell would wrap
                for g in grams(f.query)[3:]:
                    for _ in range(8):
                        lib.row([lib.filler(g)], [1.0])
    tail = sum((f.n - f.n // 2) * (1 + (3 * FILL if f.fill else 0)) for f in lib.families if f.split)
    while pad_to and len(lib.words) // row_size < pad_to - tail:
        lib.row([lib.filler()], [1.0])
    for f in lib.families:
        if f.split:
            put(f, f.n // 2, f.n)
    return lib.finish()


def lib_n1():
    return single_lib("n1", [family_n(n) for n in (600, 257, 192)], row_size=2, seed=11)


def lib_n2():
    return single_lib("n2", [family_n(n) for n in (320, 256, 255, 193)], seed=21)


def lib_n3():
    return single_lib("n3", [family_n(n) for n in (1, 63, 64, 65, 127, 128, 129)] + [family_p()], seed=31)


E_ROWS = 36000  # libraries e1 and o3 are padded to this many rows: a split family's halves are bit 15 of the key rank apart


def lib_o1():
    return single_lib("o1", [families_o()[0], family_t2()], row_size=2, seed=12)


def lib_o2():
    return single_lib("o2", [families_o()[1], families_b()[0]], seed=22)


def lib_o3():
    return single_lib("o3", [families_o()[2], families_b()[1]], seed=32, pad_to=E_ROWS)


E_LIMITS = LIMITS + (3, 4, 20, 100, 101)  # B1: bins 2 and 3 of lane 0; Ea: its last but one; Ec: the ends of runs


def lib_e1(row_size=2):
    """Row size 2 with every alias missing, so that a flag twin can add a far row with an alias."""
    return single_lib("e1", [family_ea(), family_eb(), family_ed(), family_ee(), families_b()[2]], row_size=row_size,
                      seed=13, pad_to=E_ROWS)


def lib_e2():
    return single_lib("e2", [family_ec(), family_t()], row_size=2, seed=23)


def lib_d():
    fams = [family_n(n, spread=False) for n in N_SIZES if n >= 192]
    fams += families_o(spread=False) + [family_ec(spread=False)] + families_b(spread=False)
    lib = single_lib("d", fams, dense=True, seed=14)
    return lib


M_KEYS, M_PLAIN = 300, 60


def _put_m(lib, m):
    m.pair_weights = ([1.0 + j / 512 for j in range(M_KEYS)], [1.6 - j / 512 for j in range(M_KEYS)])
    for j in range(M_KEYS):
        lib.row([lib.filler(), m.targets[0], m.targets[1]], [1.0, m.pair_weights[0][j], m.pair_weights[1][j]])
    ws = lib.fillers_of(m, 2)  # (M0 and M1 are neighbours: two targets' fillers before the next one)
    for k in range(0, len(ws), 3):
        lib.row(ws[k:k + 3], [1.0] * 3)
    for i in range(2, m.n):
        lib.row([lib.filler(), m.targets[i]], [1.0, m.weights[i]])
        ws = lib.fillers_of(m)
        for k in range(0, len(ws), 3):
            lib.row(ws[k:k + 3], [1.0] * 3)


def family_m(**kw):
    """The alias words M0 (weights ascending over its 300 keys) and M1 (descending) in the rows of 300 keys: two
    survivors of 300 pairs each, a trim inside the pair loop; then 60 keys with one ordinary target each."""
    return Family("M", [1.0, 1.0] + _shuffled([1.0 + i / 256 for i in range(M_PLAIN)], 15), **kw)


UO_TERMS, UO_KEYS, UT_TERMS, UT_KEYS = 120, 5, 130, 3


def lib_u():
    """Rows of a key and two aliases, no fillers, every list at most 135 postings. N1..N129 and Ea as keys
    without aliases; family M; and two families whose records come from several keys per alias word, since a
    list of more than 135 targets would give the index 16 buckets: Uo, 120 words under 5 keys each, the 600
    weights descending in order of arrival (refills, and tau prunes what follows); Ut, 130 words under 3 keys
    each (the last two words arrive in a third batch of 64 terms, after the first refill), every weight the library's largest (the bound fl(w_max * s) ties tau), the last key one character
    shorter: it arrives last, ties tau's score and has the best key rank of all."""
    fams = [family_n(n, spread=False) for n in N_SIZES if n <= 129] + [family_ea()]
    m = family_m(spread=False)
    uo = Family("Uo", [1.0] * UO_TERMS, spread=False)
    ut = Family("Ut", [W_MAX] * UT_TERMS, spread=False)
    lib = Lib("u", fams + [m, uo, ut], row_size=3, seed=15)
    for f in fams:
        for i in range(f.n):
            lib.row([f.targets[i]], [f.weights[i]])
    _put_m(lib, m)
    uo.records, ut.records = UO_TERMS * UO_KEYS, UT_TERMS * UT_KEYS
    for t in range(UO_TERMS):
        for j in range(UO_KEYS):
            lib.row([lib.filler(), uo.targets[t]], [1.0, 1.9 - (UO_KEYS * t + j) / 1024])
    for t in range(UT_TERMS):
        for j in range(UT_KEYS):
            key = lib.filler()
            lib.row([key[:8] if (t, j) == (UT_TERMS - 1, UT_KEYS - 1) else key, ut.targets[t]], [1.0, W_MAX])
    return lib.finish()


A_KEYS = 400


def lib_a():
    """A1: key k's row holds both aliases. A2: key k has a row with its first alias at the head of the
    library and a row with its second alias at its end. Weights by key number mod 10 (D_WEIGHTS): better
    first, better second, both alike, a negative beside a positive. Fillers come as whole rows (a key and two
    aliases, each holding one prefix gram)."""
    a1 = Family("A1", [D_WEIGHTS[k % 10][j] for k in range(A_KEYS) for j in range(2)])
    a2 = Family("A2", [D_WEIGHTS[k % 10][0] for k in range(A_KEYS)] + [D_WEIGHTS[k % 10][1] for k in range(A_KEYS)],
                split=True)
    m = family_m()
    lib = Lib("a", [a1, a2, m], row_size=3, seed=16)
    keys2 = [lib.filler() for _ in range(A_KEYS)]

    def filler_rows(f, k):
        ws = lib.fillers_of(f, k)
        for i in range(0, len(ws), 3):
            lib.row(ws[i:i + 3], [1.0] * 3)

    for k in range(A_KEYS):
        lib.row([keys2[k], a2.targets[k]], [1.0, a2.weights[k]])
        filler_rows(a2, 1)
    for k in range(A_KEYS):
        lib.row([lib.filler(), a1.targets[2 * k], a1.targets[2 * k + 1]], [1.0, a1.weights[2 * k], a1.weights[2 * k + 1]])
        filler_rows(a1, 3)  # (the two aliases are neighbours: one more set)
    _put_m(lib, m)  # family M with fillers behind its ordinary targets, for the main launch and the heavy list
    for k in range(A_KEYS):
        lib.row([keys2[k], None, a2.targets[A_KEYS + k]], [1.0, 1.0, a2.weights[A_KEYS + k]])
        filler_rows(a2, 1)
    return lib.finish()


A_LIMITS = (1, 2, 64, 128)

# ---- R: rank lists -----------------------------------------------------------------------------------
R_LENGTHS = (300, 200, 129, 128, 127, 100, 65, 64, 63, 10)  # the one-hit rows of the query's 10 lists
R_MULTI = {"some": 40, "full": 150, "none": 0}
R_EVERY = 16  # a multi-hit target every 16th round of one-hit rows: at most 21 among the 328 postings that a
# cmin-2 part can hold of the first list (55 of the 64 lanes at the very most: 165 >> 1 chunks)
R_PART = 4 * ((3 * 55) >> 1)


def r_lengths(kind):
    return (R_EVERY * R_MULTI[kind],) + R_LENGTHS[1:] if R_MULTI[kind] else R_LENGTHS


def lib_r(weight=None):
    """One weight (None: the default 1.0) and one word per row. Three queries of 10 distinct grams; list j of
    each has r_lengths[j] one-hit rows (a filler around gram j), laid out round-robin so every list starts
    at the lowest key ranks. The multi-hit targets (the query's first 5 characters and a suffix: 3 hits, in
    the first three lists) stand between the rounds, one every 16th round, so tier 1a's cmin-2 parts stay
    within 64 candidate entries and the query reaches emit_rank_prefix: 40 for "some" (8 of them among the
    first 128 key ranks of the first list, where kset must drop their one-hit stand-ins), 150 (more than the
    largest limit: the multi-hit top-L is full before the prefix merge; its first list has 2,400 one-hit
    rows) for "full", none for "none"."""
    lib = Lib("r", [], seed=17)
    lib.queries = {}
    for kind, n_multi in R_MULTI.items():
        while True:
            q = "".join(lib.rng.choices(PLANT, k=12))
            g = grams(q)
            if len(set(g)) == 10 and not set(g) & lib.used:
                break
        lib.used |= set(g)
        lib.queries[kind] = q
        lens = r_lengths(kind)
        for i in range(max(lens)):
            if i % R_EVERY == 0 and i // R_EVERY < n_multi:
                lib.row([q[:5] + _digits(i // R_EVERY, SUF, 4)], [1.0])
            for j, n in enumerate(lens):
                if i < n:
                    lib.row([lib.filler(g[j])], [1.0])
    lib.weights = None if weight is None else [weight] * len(lib.words)
    return lib.finish()


MAKERS = {"n1": lib_n1, "n2": lib_n2, "n3": lib_n3, "o1": lib_o1, "o2": lib_o2, "o3": lib_o3, "e1": lib_e1, "e2": lib_e2,
          "d": lib_d, "u": lib_u, "a": lib_a}
SPREAD = ("n1", "n2", "n3", "o1", "o2", "o3", "e1", "e2", "a")
# (base library, twin) pairs: every twin of e1, and those that flip a flag of libraries whose families refill
# the buffer (o1 is not monotone to begin with: T2's short key; a has neither unique keys nor monotone ids)
TWIN_CASES = [("e1", k) for k in ("alias", "shared", "short", "huge")] + [
    ("e2", "short"), ("e2", "huge"), ("o1", "alias"), ("o1", "huge"), ("n1", "alias"), ("n1", "shared"), ("n1", "short"),
    ("a", "huge")]


def limits_of(name):
    if name == "n3":  # P: cuts between its groups of six equal scores
        return LIMITS + (6, 7, 12, 13, 24, 25)
    return E_LIMITS if name[0] == "e" or name in ("o2", "o3") else A_LIMITS if name == "a" else LIMITS


def survivors(f):
    """The terms of Q_f that pass cmin 3 and cmin 2: the targets, and the query's own row where it has one."""
    return f.n + (1 if f.tail != TAIL else 0)


def part_entries(plain, q, cmin, width=None, lists=None):
    """The most candidate entries (postings of terms with cmin hits or more) that a main-launch part of `q` can
    hold: over every list of q, every window of the postings a part takes of one list (halved at cmin 2),
    the hits of the window's candidate terms."""
    counts = plain.counts(q)
    width = width or PART_POSTINGS >> (1 if cmin == 2 else 0)
    worst = 0
    for x in lists or dict.fromkeys(grams(q)):
        lst = plain.lists.get(x, ())
        hit = [counts[t] if counts[t] >= cmin else 0 for t in lst]
        run = sum(hit[:width])
        worst = max(worst, run)
        for j in range(width, len(hit)):
            run += hit[j] - hit[j - width]
            worst = max(worst, run)
    return worst


# ---- flag twins ------------------------------------------------------------------------------------------
TWINS = ("alias", "shared", "short", "huge")


def twin(lib, kind):
    """`lib` and one or two far rows over V and W, which no query touches (row size 2 at least)."""
    import copy
    t = copy.copy(lib)
    t.__dict__.pop("_model", None)
    t.name = f"{lib.name}+{kind}"
    t.words, t.weights = list(lib.words), None if lib.weights is None else list(lib.weights)
    if kind == "alias":       # a key with two terms: keys_unique off, tk_identity still on
        t.row(["VVVWWWVVV", "WWWVVVWWW"], [1.0, 1.0])
    elif kind == "shared":    # one alias word under two keys: tk_identity off
        t.row(["VVVWWWVVV", "WVWVWVWVW"], [1.0, 1.0])
        t.row(["WWWVVVWWW", "WVWVWVWVW"], [1.0, 1.0])
    elif kind == "short":     # a last term whose key is shorter than every other: tk_monotone off
        t.row(["VVWWVVWW"], [1.0])
    elif kind == "huge":      # w_max = 1e30: every prune bound is loose
        t.row(["VVVWWWVVV"], [1e30])
    elif kind == "weight":    # (library r) a second weight: rank lists off
        t.weights = [1.0 if lib.weights is None else lib.weights[0]] * len(t.words)
        t.row(["VVVWWWVVV"], [0.5])
    else:
        raise ValueError(kind)
    return t.finish()


def negative(lib):
    """Every weight negative or zero-scoring (w_max <= 0): all scores are +0 and the key rank alone cuts."""
    import copy
    t = copy.copy(lib)
    t.__dict__.pop("_model", None)
    t.name = f"{lib.name}+negative"
    t.weights = [-abs(w) for w in lib.weights]
    return t


def flag_word(model):
    """ngsIndexDigest word 16 as ngs_abi.cpp's upload() derives it from the pairs: 1 keys_unique, 2 tk_identity,
    4 tk_monotone, 8 rank lists (NGS_NO_RANK_LISTS apart)."""
    seen, unique = set(), True
    for p in model.tk:
        for r, _ in p:
            unique = unique and r not in seen
            seen.add(r)
    identity = all(len(p) == 1 for p in model.tk)
    mono, prev = True, -1
    for p in model.tk:
        if p:
            mono = mono and min(r for r, _ in p) > prev
            prev = max(r for r, _ in p)
    ws = {w for p in model.tk for _, w in p}
    rank = unique and identity and len(ws) == 1 and float(build_ref.bits_f32(next(iter(ws)))) <= 200.0
    return (1 if unique else 0) | (2 if identity else 0) | (4 if mono else 0) | (8 if rank else 0)


def w_max(model):
    return max([0.0] + [build_ref.bits_f32(w) for p in model.tk for _, w in p])


# ---- the plain model ---------------------------------------------------------------------------------------
class Plain:
    """Answers from the build model's terms and pairs alone: counts by a scan of the lists, calcScore's max per
    key, a full sort by (score descending, key rank ascending), the first `limit`."""

    def __init__(self, lib):
        self.lib, self.m = lib, lib.model()
        self.terms = [bytes(t).decode() for t in self.m.terms]
        self.keys = [bytes(k) for k in self.m.keys]
        self.lists = {}
        for i, t in enumerate(self.terms):
            for x in set(grams(t)):
                self.lists.setdefault(x, []).append(i)

    def counts(self, q):
        c = {}
        for x in grams(q):
            for t in self.lists.get(x, ()):
                c[t] = c.get(t, 0) + 1
        return c

    def records(self, q, thr):
        """[(term id, [(score bits, key rank), ...])] in term-id order: every pair's record."""
        n = f32(len(q) - 2)
        out = []
        for t, c in sorted(self.counts(q).items()):
            s = f32(c) / n
            if s < f32(thr):
                continue
            recs = []
            for r, wb in self.m.tk[t]:
                sb = score_bits(build_ref.bits_f32(wb), s)
                if float(s) > 0.999 and self.keys[r] == q.encode():
                    sb = bits(f32(100.0))
                recs.append((sb, r))
            out.append((t, recs))
        return out

    def best(self, q, thr):
        best = {}
        for _, recs in self.records(q, thr):
            for sb, r in recs:
                if r not in best or from_bits(sb) > from_bits(best[r]):
                    best[r] = sb
        return sorted(((sb, r) for r, sb in best.items()), key=lambda x: (-float(from_bits(x[0])), x[1]))

    def answer(self, q, thr, limit):
        a = self.best(q, thr)
        return [(self.keys[r], sb) for sb, r in (a[:limit] if limit else a)]


# ---- the buffer model and its mutants ------------------------------------------------------------------------
MUTATIONS = ("tie_out", "lt_kth", "dedup_first", "prune_le")  # (and rank_prefix_model's skip_kset)


def buffer_model(terms, L, mutation=None):
    """The running top-L as emit_query / wave_emit keep it, on `terms` = [(bound enc, [(score bits, key rank),
    ...])] in order of arrival: 64 terms per batch, each pruned against tau (term_pairs), their pairs appended
    lane by lane, a trim (dedup by key keeping the best, the L smallest, tau = the L-th) whenever 64 more
    records would not fit, and a final flush. Returns ([(score bits, key rank)], refills).

    Mutations, one at a time: "prune_le" prunes a term whose bound ties tau (term_pairs with <=), "tie_out"
    drops a record that ties tau's score whatever its key rank (raised_cmin's rule without tk_monotone; the
    inverse, admitting a tie at tau, only adds records that the next trim cuts again, so no answer can show it),
    "lt_kth" keeps the records < the L-th instead of <=, "dedup_first" keeps a key's first-arrived record."""
    NO = 2**64 - 1
    buf, tau, refills = [], NO, 0

    def trim(final=False):
        nonlocal buf, tau, refills
        refills += 0 if final else 1
        by_key = {}
        for rec in buf:  # in order of arrival
            k = rec & 0xFFFFFFFF
            if k not in by_key or (mutation != "dedup_first" and rec < by_key[k]):
                by_key[k] = rec
        recs = sorted(by_key.values())
        if len(recs) >= L:
            kth = recs[L - 1]
            recs = [r for r in recs if (r < kth if mutation == "lt_kth" else r <= kth)]
            tau = kth
        buf = recs

    for base in range(0, len(terms), 64):
        lanes = []
        for bound, recs in terms[base:base + 64]:
            te = ~(tau >> 32) & 0xFFFFFFFF
            pruned = tau != NO and (bound <= te if mutation == "prune_le" else bound < te)
            lanes.append([] if pruned else [record(sb, r) for sb, r in recs])
        for p in range(max(map(len, lanes), default=0)):
            if len(buf) + 64 > CAND:
                trim()
            for recs in lanes:
                if p < len(recs):
                    rec = recs[p]
                    if mutation == "tie_out" and tau != NO and rec >> 32 == tau >> 32:
                        continue
                    if rec < tau:
                        buf.append(rec)
    trim(final=True)
    return [(enc - 1 if enc > 1 else 0, r) for enc, r in ((~(x >> 32) & 0xFFFFFFFF, x & 0xFFFFFFFF) for x in buf)], refills


def arrival(plain, q, thr):
    """buffer_model's input for a query: every surviving term with its bound fl(w_max * s)."""
    wm = w_max(plain.m)
    n = f32(len(q) - 2)
    counts = plain.counts(q)
    out = []
    for t, recs in plain.records(q, thr):
        ub = f32(wm) * (f32(counts[t]) / n)
        out.append((enc_of(bits(ub) if ub > 0 else 0), recs))
    return out


# ---- the rank-list shortcut, restated for the kset mutation ----------------------------------------------------
def rank_prefix_model(plain, q, L, skip_kset=False):
    """emit_rank_prefix on a one-weight library at threshold 0: the multi-hit records' top-L, then every
    list's first L key ranks as one-hit records, without those whose key is in the multi-hit top-L (kset)."""
    counts = plain.counts(q)
    n = f32(len(q) - 2)
    w = build_ref.bits_f32(plain.m.tk[0][0][1])
    multi = sorted(record(score_bits(w, f32(c) / n), plain.m.tk[t][0][0]) for t, c in counts.items() if c >= 2)[:L]
    kset = {r & 0xFFFFFFFF for r in multi}
    one = score_bits(w, f32(1) / n)
    recs = list(multi)
    for x in dict.fromkeys(grams(q)):
        ranks = sorted(plain.m.tk[t][0][0] for t in plain.lists.get(x, ()))[:L]
        recs += [record(one, r) for r in ranks if skip_kset or r not in kset]
    if not skip_kset:
        recs = sorted(set(recs))
    else:
        recs = sorted(recs)  # a multi-hit key's stand-in stays beside its real record
    return [(plain.keys[r & 0xFFFFFFFF], (~(r >> 32) & 0xFFFFFFFF) - 1 if (~(r >> 32) & 0xFFFFFFFF) > 1 else 0)
            for r in recs[:L]]
