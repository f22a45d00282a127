"""A seeded corpus of valid BGZF members for the inflate (iss_inflate_core.h on the host, k_bgzf_inflate on the device), the damaged
streams made from it, and the rule that judges a damaged stream by zlib.  tests/inflate_cases.py pins one member per stated cause; this
module samples the cross products: code shape x block order x match geometry x the place where a 16 KiB piece leaves the ring.

corpus() draws every member from four independent plans -- code shapes (complete codes as random Kraft splits with a chosen longest
code, HLIT / HDIST / HCLEN over their ranges, the incomplete sets zlib takes, the same length vector written with different mixes of
plain lengths, 16, 17 and 18), block plans (one to six blocks in every order, empty blocks of each type), token plans (matches by
distance class, lengths at both ends of every extra-bits class) and size plans (tiny, small, boundary, last pieces).  Seeds are
fixed; nothing reads the clock or the environment, so the bytes are the same everywhere (digest()).  ledger() says what the corpus
holds, found by walking the members' blocks and tokens, not by trusting the plans.

Three things the format itself rules out, so the ledger words them as follows:
  - HCLEN = 4 gives the code-length code the symbols 16, 17, 18 and 0 only: every length is 0, there is no end-of-block code, the block
    is bad.  Valid members have HCLEN 5 .. 19; HCLEN 4 is among the damaged streams (hclen_4_stream).
  - A match is 3 .. 258 bytes.  The cell "starts at 16384 k - a, ends at 16384 k + b" is one match where 3 <= a + b <= 258, two matches
    back to back where a + b > 258 or a + b = 0 (one ends at the boundary, the next starts there), and where a + b is 1 or 2 no
    sequence of matches can hold both ends: those five cells count a match that starts at 16384 k - a and one that ends at 16384 k + b
    in two members.
  - length > distance needs distance < 258, length < distance needs distance > 3: the distances 1, 2, 3 are seen with length >
    (and, for 3, =) only, the far distances (above 32768 - 258) with length < only.

damage() and verdict(): see their docstrings; DESIGN.md section 27."""
import hashlib
import random
import struct
import zlib

import inflate_cases as IC

PIECE = 16384
AB = (0, 1, 2, 3, 63, 64, 65, 257)
NEAR = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257)
FAR = 32768 - 258
PRODUCERS = ("match", "stored", "lit")
N_TINY_PER_SIZE, N_SMALL = 30, 1200
MAX_BASE_PAYLOAD = 1500


# ---------------------------------------------------------------------------------------------------- code shapes
def kraft_split(rnd, n, longest):
    """n code lengths of a complete code whose longest code has `longest` bits: a spine 1, 2, .., longest, longest, then random leaves
    split until there are n.  (longest + 1 <= n <= 2^longest; for longest 1: n = 2.)"""
    lens = list(range(1, longest)) + [longest, longest]
    assert len(lens) <= n <= (1 << longest), (n, longest)
    open_ = [i for i, l in enumerate(lens) if l < longest]
    while len(lens) < n:
        k = rnd.randrange(len(open_))
        i = open_[k]
        lens[i] += 1
        lens.append(lens[i])
        if lens[i] == longest:
            open_[k] = open_[-1]
            open_.pop()
        else:
            open_.append(len(lens) - 1)
    assert IC.kraft(lens) == 1.0 and max(lens) == longest
    return lens


def draw_code(rnd, size, required, longest, pool=None):
    """A length vector of `size` entries: a complete code with the longest code `longest` over the required symbols and random others
    (from `pool`, default all)."""
    required = sorted(required)
    have = set(required)
    others = [s for s in (range(size) if pool is None else pool) if s not in have and s < size]
    lo, hi = max(longest + 1, len(required), 2), min(len(required) + len(others), 1 << longest)
    assert lo <= hi, (size, len(required), longest)
    n = rnd.choice([lo, hi, rnd.randint(lo, hi), min(hi, lo + int(rnd.expovariate(1 / 12.0)))])
    syms = required + rnd.sample(others, n - len(required))
    split = kraft_split(rnd, n, longest)
    rnd.shuffle(split)
    lens = [0] * size
    for s, l in zip(syms, split):
        lens[s] = l
    return lens


def min_longest(n_symbols):
    l = 1
    while (1 << l) < n_symbols:
        l += 1
    return l


def encode_ops(rnd, lens, p_zero, p_rep):
    """The length vector as header ops: runs of zeros as 17 / 18 with probability p_zero, a run of the length before (zero too) as 16
    with probability p_rep, plain lengths otherwise."""
    ops, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        run = 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3 and rnd.random() < p_zero:
            if run >= 11 and rnd.random() < 0.7:
                r = rnd.choice([11, min(138, run), rnd.randint(11, min(138, run))])
                ops.append(("z18", r))
            else:
                r = rnd.choice([3, min(10, run), rnd.randint(3, min(10, run))])
                ops.append(("z17", r))
            i += r
        elif i > 0 and lens[i - 1] == v and run >= 3 and rnd.random() < p_rep:
            r = rnd.choice([3, min(6, run), rnd.randint(3, min(6, run))])
            ops.append(("rep16", r))
            i += r
        else:
            ops.append(("len", v))
            i += 1
    return ops


def ops_symbols(ops):
    return set({"rep16": 16, "z17": 17, "z18": 18}.get(op[0], op[1]) for op in ops)


def draw_cl_code(rnd, ops, longest=None, pool=None):
    """(cl_lens, hclen) of a complete code-length code over the symbols the ops use."""
    used = ops_symbols(ops)
    if len(used) == 1:
        used.add(rnd.choice([s for s in (pool or range(19)) if s not in used]))  # a complete code has two codes at least
    lo = min_longest(len(used))
    longest = rnd.randint(lo, 7) if longest is None else max(lo, longest)
    while longest + 1 > (19 if pool is None else len(set(pool) | used)):
        longest -= 1
    cl = draw_code(rnd, 19, used, longest, pool)
    least = max(4, 1 + max(i for i in range(19) if cl[IC.CL_ORDER[i]]))
    return cl, rnd.choice([least, least, 19, rnd.randint(least, 19)])


# ---------------------------------------------------------------------------------------------------- token plans
def length_ends():
    out = []
    for s in range(29):
        out += [IC.LEN_BASE[s], min(258 if s == 28 else 257, IC.LEN_BASE[s] + (1 << IC.LEN_EXTRA[s]) - 1)]
    return sorted(set(out))


LENGTH_ENDS = length_ends()


def draw_tokens(rnd, pos, budget, cap_l, cap_d, lit_pool, p_lit=0.45, max_tokens=400):
    """Literal and match tokens for at most `budget` bytes behind `pos` bytes of history, over at most cap_l literal/length symbols and
    cap_d distance symbols.  Matches are drawn by class: a named distance with a length below, equal to or above it; distance =
    position; a length at an end of its extra-bits class; anything."""
    tokens, used_l, used_d, end = [], set(), set(), pos + budget

    def may(used, sym, cap):
        return sym in used or len(used) < cap

    def literal():
        pool = [c for c in lit_pool if c in used_l] if len(used_l) >= cap_l else lit_pool
        if not pool:
            return False
        c = rnd.choice(pool)
        used_l.add(c)
        tokens.append(("lit", c))
        return True

    while pos < end and len(tokens) < max_tokens:
        room = end - pos
        done = False
        if pos > 0 and room >= 3 and cap_d and rnd.random() >= p_lit:
            for _ in range(4):
                kind = rnd.choice(("near", "near", "pos", "ends", "any"))
                if kind == "near":
                    d = rnd.choice(NEAR)
                    rel = rnd.choice("<=>")
                    n = rnd.randint(3, d - 1) if rel == "<" and d > 3 else d if rel == "=" else rnd.randint(d + 1, 258) if d < 258 else 258
                elif kind == "pos":
                    d, n = pos, rnd.choice([3, 258, rnd.randint(3, 258)])
                elif kind == "ends":
                    n = rnd.choice(LENGTH_ENDS)
                    d = rnd.choice([n - 1, n, n + 1, rnd.randint(1, pos)])
                else:
                    n, d = rnd.randint(3, 258), rnd.randint(1, pos)
                if not (3 <= n <= min(258, room) and 1 <= d <= min(pos, 32768)):
                    continue
                ls, ds = IC.length_symbol(n)[0], IC.distance_symbol(d)[0]
                if may(used_l, ls, cap_l) and may(used_d, ds, cap_d):
                    used_l.add(ls)
                    used_d.add(ds)
                    tokens.append(("match", n, d))
                    pos += n
                    done = True
                    break
        if not done:
            if not literal():
                break
            pos += 1
    return tokens, used_l, used_d


def filler(rnd, pos, target):
    """Matches, 258 bytes wherever they fit, from pos (> 0) to exactly target; distances by class, the far ones once the position has
    passed 32768."""
    tokens = []
    while pos < target:
        r = target - pos
        n = 258 if r > 516 else r // 2 if r > 258 else r
        assert 3 <= n <= 258, (pos, target)
        pick = rnd.randrange(8)
        d = (rnd.randint(FAR + 1, 32768) if pos > 32768 and pick < 3 else rnd.choice(NEAR) if pick < 5 else min(pos, 32768) if pick == 5
             else rnd.randint(1, min(pos, 32768)))
        d = min(d, pos)
        tokens.append(("match", n, d))
        pos += n
    return tokens


def used_symbols(tokens):
    ul, ud = set(), set()
    for t in tokens:
        if t[0] == "lit":
            ul.add(t[1])
        elif t[0] == "match":
            ul.add(IC.length_symbol(t[1])[0])
            ud.add(IC.distance_symbol(t[2])[0])
    return ul, ud


# ---------------------------------------------------------------------------------------------------- blocks
def dyn_block(rnd, tokens, l_longest=None, d_longest=None, mode=None, special=None):
    """A dynamic block around the tokens: codes over the symbols they use, the header written in a drawn mix."""
    ul, ud = used_symbols(tokens)
    ul.add(256)
    if special == "one_lit":  # the incomplete literal/length set zlib takes: the end-of-block code alone, one bit
        assert not tokens
        lit_lens = [0] * rnd.randint(257, 286)
        lit_lens[256] = 1
    else:
        lo = min_longest(len(ul))
        l_longest = max(lo, l_longest or rnd.randint(lo, 15))
        hlit = rnd.randint(max(257, max(ul) + 1), 286)
        lit_lens = draw_code(rnd, hlit, ul, l_longest)
    if special == "one_dist":  # the incomplete distance set zlib takes: one code of one bit
        assert len(ud) <= 1
        dist_lens = [0] * rnd.randint(max(ud) + 1 if ud else 1, 30)
        dist_lens[max(ud) if ud else rnd.randrange(len(dist_lens))] = 1
    elif special == "no_dist" or (not ud and special == "one_lit"):
        assert not ud
        dist_lens = [0] * rnd.randint(1, 30)
    else:
        lo = min_longest(max(2, len(ud)))
        d_longest = max(lo, d_longest or rnd.randint(lo, 15))
        hdist = rnd.randint(max(d_longest + 1, max(ud) + 1 if ud else 1, 2), 30)
        dist_lens = draw_code(rnd, hdist, ud, d_longest)
    mode = mode or rnd.choice(("plain", "runs", "mixed", "mixed"))
    p_zero, p_rep = {"plain": (0.0, 0.0), "runs": (1.0, 1.0), "mixed": (rnd.random(), rnd.random())}[mode]
    ops = encode_ops(rnd, lit_lens + dist_lens, p_zero, p_rep)
    cl_lens, hclen = draw_cl_code(rnd, ops)
    return {"type": "dyn", "tokens": tokens, "lit_lens": lit_lens, "dist_lens": dist_lens, "ops": ops, "cl_lens": cl_lens, "hclen": hclen}


def band_block(rnd, hclen, mode):
    """A dynamic block whose header has exactly this HCLEN (5 .. 19): literal/length lengths from the first hclen symbols of the
    code-length order only, the last of them included; no distance code; literals."""
    allowed = IC.CL_ORDER[:hclen]
    new = allowed[-1]
    multiset = [8] * 256
    if new < 8:
        multiset = [8] * (256 - (1 << (8 - new))) + [new]
    elif new > 8:
        multiset = [8] * 255 + list(range(9, new)) + [new, new]
    assert IC.kraft(multiset) == 1.0 and all(l in allowed for l in multiset)
    hlit = rnd.randint(max(257, len(multiset)), 286)
    syms = [256] + rnd.sample([s for s in range(hlit) if s != 256], len(multiset) - 1)
    rnd.shuffle(multiset)
    lit_lens = [0] * hlit
    for s, l in zip(syms, multiset):
        lit_lens[s] = l
    lits = [s for s in syms if s < 256]
    tokens = [("lit", rnd.choice(lits)) for _ in range(rnd.randint(0, 60))]
    dist_lens = [0] * rnd.randint(1, 30)
    p = {"plain": (0.0, 0.0), "runs": (1.0, 1.0), "mixed": (0.5, 0.5)}[mode]
    ops = encode_ops(rnd, lit_lens + dist_lens, *p)
    cl_lens, _ = draw_cl_code(rnd, ops, pool=[s for s in allowed])
    cl_used = [i for i in range(19) if cl_lens[IC.CL_ORDER[i]]]
    assert max(cl_used) + 1 == hclen
    return {"type": "dyn", "tokens": tokens, "lit_lens": lit_lens, "dist_lens": dist_lens, "ops": ops, "cl_lens": cl_lens, "hclen": hclen}


def assemble(blocks):
    """(payload, data, bit offset of every block header) of the blocks; the last one is final."""
    w, data, at = IC.BitWriter(), b"", []
    for i, b in enumerate(blocks):
        final = i == len(blocks) - 1
        at.append(w.pos())
        if b["type"] == "stored":
            IC.stored_block(w, b["data"], final=final)
            data += b["data"]
            continue
        if b["type"] == "fixed":
            IC.fixed_block(w, b["tokens"] + [("end",)], final=final)
        else:
            IC.dynamic_header(w, len(b["lit_lens"]), len(b["dist_lens"]), b["ops"], b["cl_lens"], final, b["hclen"])
            IC.put_tokens(w, b["tokens"] + [("end",)], b["lit_lens"], b["dist_lens"])
        data += IC.play(b["tokens"], data)
    return w.done(), data, at


def make(name, plan, blocks):
    payload, data, at = assemble(blocks)
    return {"name": name, "plan": plan, "member": IC.member(payload, data), "data": data, "status": IC.OK, "blocks": blocks,
            "header_bits": at}


# ---------------------------------------------------------------------------------------------------- small and tiny members
PAIRS = [(a, b) for a in ("stored", "fixed", "dyn") for b in ("stored", "fixed", "dyn")]


def small_member(rnd, index, budget, name, plan):
    n_blocks = 1 + index % 6 if index % 7 else rnd.randint(1, 6)
    types = [rnd.choice(("stored", "fixed", "dyn")) for _ in range(n_blocks)]
    if n_blocks >= 2:
        at = rnd.randrange(n_blocks - 1)
        types[at:at + 2] = PAIRS[index % 9]
    empty = [rnd.random() < 0.18 for _ in types]
    if index % 11 == 0:
        empty[-1] = True
    if index % 13 == 0:
        empty[0] = True
    live = [i for i in range(n_blocks) if not empty[i]]
    cuts = sorted(rnd.randint(0, budget) for _ in range(max(0, len(live) - 1)))
    share = dict(zip(live, [b - a for a, b in zip([0] + cuts, cuts + [budget])]))
    blocks, pos = [], 0
    for i, t in enumerate(types):
        n = share.get(i, 0)
        if t == "stored":
            blocks.append({"type": "stored", "data": IC.noise(n, rnd.getrandbits(30)) if rnd.random() < 0.5 else
                           bytes(bytearray(rnd.choice(b"ACGT\n") for _ in range(n)))})
            pos += n
            continue
        l_longest = 1 + (index + i) % 15 if t == "dyn" else None
        d_longest = 1 + (index // 15 + i) % 15 if t == "dyn" else None
        special = None
        if t == "dyn" and (index + i) % 17 == 0:
            special = ("one_dist", "no_dist", "one_lit")[(index // 17 + i) % 3]
        cap_l = 300 if t == "fixed" else (1 << l_longest) - 1
        cap_d = 30 if t == "fixed" else 1 << d_longest
        if special == "one_dist":
            cap_d = 1
        elif special == "no_dist":
            cap_d = 0
        elif special == "one_lit":
            n = 0
        pool = list(range(256)) if rnd.random() < 0.3 else rnd.sample(range(256), rnd.choice((1, 2, 4, 20, 90)))
        tokens, ul, ud = draw_tokens(rnd, pos, n, cap_l, cap_d, pool, p_lit=rnd.choice((0.1, 0.45, 0.8))) if n else ([], set(), set())
        if special == "one_dist" and not ud and pos + len(tokens) == 0:
            special = "no_dist"
        pos += sum(1 if x[0] == "lit" else x[1] for x in tokens)
        if t == "fixed":
            blocks.append({"type": "fixed", "tokens": tokens})
        else:
            blocks.append(dyn_block(rnd, tokens, l_longest, d_longest, special=special))
    return make(name, plan, blocks)


def cl1_member(rnd, name):
    """The code-length code with one-bit codes: lengths 0 and 8 only, plain."""
    lit_lens = [0] + [8] * 256
    tokens = [("lit", rnd.randint(1, 255)) for _ in range(40)]
    cl = [0] * 19
    cl[0] = cl[8] = 1
    ops = IC.plain_ops(lit_lens + [0])
    return make(name, "small", [{"type": "dyn", "tokens": tokens, "lit_lens": lit_lens, "dist_lens": [0], "ops": ops, "cl_lens": cl,
                                 "hclen": 5}])


# ---------------------------------------------------------------------------------------------------- boundary members
def coded(rnd, tokens, index):
    if index % 2:
        return {"type": "fixed", "tokens": tokens}
    return dyn_block(rnd, tokens, l_longest=9 + index % 7, d_longest=5 + index % 11)


def boundary_member(rnd, index, producer, cells, total, ending, name):
    """A member of `total` bytes, mostly 258-byte matches and a few stored runs, in which `producer` starts at 16384 k - a and ends at
    16384 k + b for every (k, a, b) of cells; `ending`: what produces the last byte."""
    blocks = [{"type": "stored", "data": IC.noise(300 + rnd.randrange(400), rnd.getrandbits(30))}]
    pos = len(blocks[0]["data"])
    tokens = []

    def close():
        if tokens:
            blocks.append(coded(rnd, list(tokens), index + len(blocks)))
            del tokens[:]

    def fill(target):
        if target - pos > 3000 and rnd.random() < 0.5:  # a stored run on the way
            run = rnd.randint(1, 700)
            mid = pos + rnd.randint(3, target - pos - run - 3)
            tokens.extend(filler(rnd, pos, mid))
            close()
            blocks.append({"type": "stored", "data": IC.noise(run, rnd.getrandbits(30))})
            tokens.extend(filler(rnd, mid + run, target))
        else:
            tokens.extend(filler(rnd, pos, target))

    for k, a, b in sorted(cells):
        s, e = PIECE * k - a, PIECE * k + b
        if producer == "match":
            if a + b == 0:
                fill(s - 258)
                tokens.extend([("match", 258, rnd.choice(NEAR)), ("match", 258, min(s, 32768 - rnd.randrange(200)))])
                pos = s + 258
            elif a + b < 3:
                fill(s)
                tokens.append(("match", 258, rnd.choice(NEAR)))
                pos = s + 258
            else:
                fill(s)
                first = a + b if a + b <= 258 else min(258, a + b - 3)
                tokens.append(("match", first, min(s, rnd.choice(NEAR + (first, 32768, 32768 - a)))))
                if a + b > first:
                    tokens.append(("match", a + b - first, rnd.choice(NEAR)))
                pos = e
        elif producer == "lit":
            if a + b == 0:
                fill(s - 5)
                tokens.extend(("lit", rnd.getrandbits(8)) for _ in range(5))
                close()
                tokens.extend(("lit", rnd.getrandbits(8)) for _ in range(5))
                pos = s + 5
            else:
                fill(s)
                tokens.extend(("lit", rnd.getrandbits(8)) for _ in range(a + b))
                pos = e
        else:
            if a + b == 0:
                fill(s - 7)
                close()
                blocks.append({"type": "stored", "data": IC.noise(7, rnd.getrandbits(30))})
                blocks.append({"type": "stored", "data": IC.noise(7, rnd.getrandbits(30))})
                pos = s + 7
            else:
                fill(s)
                close()
                blocks.append({"type": "stored", "data": IC.noise(a + b, rnd.getrandbits(30))})
                pos = e
    if ending == "match":
        fill(total - 258)
        tokens.append(("match", 258, min(total - 258, 32768)))
    elif ending == "lit":
        fill(total - 1)
        tokens.append(("lit", 0x5a))
    else:
        fill(total - 300)
        close()
        blocks.append({"type": "stored", "data": IC.noise(300, rnd.getrandbits(30))})
    close()
    m = make(name, "boundary", blocks)
    assert len(m["data"]) == total, (name, len(m["data"]), total)
    return m


def boundary_members(rnd):
    out = []
    combos = [(a, b) for a in AB for b in AB]
    endings = ("match", "stored", "lit")
    for p, producer in enumerate(PRODUCERS):
        for i in range(64):
            cells = [(k, ) + combos[(i + 21 * (k - 1)) % 64] for k in (1, 2, 3)]
            total = 65536 if i % 4 else 65535
            out.append(boundary_member(rnd, i, producer, cells, total, endings[(i + p) % 3], "boundary_%s_%d" % (producer, i)))
    # last pieces of 1 .. 4, 16383 and 16384 bytes behind one, two and three whole pieces
    for j in (1, 2, 3):
        for r in (1, 2, 3, 4, 16383, 16384):
            total = PIECE * j + r
            out.append(boundary_member(rnd, j + r, "match", [], total, endings[(j + r) % 3], "last_piece_%d_%d" % (j, r)))
    return out


# ---------------------------------------------------------------------------------------------------- the corpus
_CACHE = {}


def corpus():
    if "corpus" in _CACHE:
        return _CACHE["corpus"]
    rnd = random.Random(20270)
    out = []
    for size in range(10):
        for i in range(N_TINY_PER_SIZE):
            out.append(small_member(rnd, len(out), size, "tiny_%d_%d" % (size, i), "tiny"))
    for i in range(N_SMALL):
        budget = int(2 ** rnd.uniform(3.4, 11)) if i % 10 else 2048
        out.append(small_member(rnd, len(out), min(2048, budget), "small_%d" % i, "small"))
    out.append(cl1_member(rnd, "cl_code_of_one_bit"))
    for hclen in range(5, 20):
        for mode in ("plain", "runs", "mixed"):
            out.append(make("hclen_%d_%s" % (hclen, mode), "small", [band_block(rnd, hclen, mode)]))
    out += boundary_members(rnd)
    _CACHE["corpus"] = out
    return out


def digest(members=None):
    h = hashlib.sha256()
    for m in (corpus() if members is None else members):
        h.update(struct.pack("<I", len(m["member"])) + m["member"])
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------- the ledger
def events(m):
    """[(producer, start, end)] of a member: every match, every stored block, every run of literals inside a block."""
    out, pos = [], 0
    for b in m["blocks"]:
        if b["type"] == "stored":
            if b["data"]:
                out.append(("stored", pos, pos + len(b["data"])))
            pos += len(b["data"])
            continue
        run = None
        for t in b["tokens"]:
            if t[0] == "lit":
                run = pos if run is None else run
                pos += 1
                continue
            if run is not None:
                out.append(("lit", run, pos))
                run = None
            out.append(("match", pos, pos + t[1], t[2]))
            pos += t[1]
        if run is not None:
            out.append(("lit", run, pos))
    return out


def features(m):
    """What one member holds, as a set of tags (the ledger is their union; damage() picks its base members by them)."""
    f = set()
    blocks = m["blocks"]
    f.add(("size", m["plan"]))
    for i, b in enumerate(blocks):
        final = i == len(blocks) - 1
        f.add(("header_bit", m["header_bits"][i] % 8))
        f.add(("type", b["type"]))
        if i:
            f.add(("pair", blocks[i - 1]["type"], b["type"]))
        if not (b["data"] if b["type"] == "stored" else b["tokens"]):
            f.add(("empty", b["type"], final))
        if b["type"] == "stored":
            continue
        if b["type"] == "dyn":
            ll, dl, cl = b["lit_lens"], b["dist_lens"], b["cl_lens"]
            f.add(("hlit", len(ll)))
            f.add(("hdist", len(dl)))
            f.add(("hclen", b["hclen"]))
            f.update(("lit_len", l) for l in ll if l)
            f.update(("dist_len", l) for l in dl if l)
            f.update(("cl_len", l) for l in cl if l)
            f.add(("lit_longest", max(ll)))
            f.add(("dist_longest", max(dl)))
            f.add(("cl_longest", max(cl)))
            if IC.kraft(ll) < 1.0:
                f.add(("incomplete", "lit"))
            if max(dl) == 0:
                f.add(("no_distance_code",))
            elif IC.kraft(dl) < 1.0:
                f.add(("incomplete", "dist"))
            at = 0
            for op in b["ops"]:
                n = 1 if op[0] == "len" else op[1]
                f.add(("op", op[0]))
                if op[0] != "len" and at < len(ll) < at + n:
                    f.add(("run_crosses", op[0]))
                at += n
            f.add(("ops_mix", "plain" if all(op[0] == "len" for op in b["ops"]) else "runs"))
        else:
            ll, dl = IC.FIXED_LIT, IC.FIXED_DIST
        for t in b["tokens"]:
            if t[0] == "lit":
                if ll[t[1]] > 10:
                    f.add(("beyond_direct", "lit"))
                continue
            ls, ds = IC.length_symbol(t[1])[0], IC.distance_symbol(t[2])[0]
            f.add(("len_sym", ls))
            f.add(("dist_sym", ds))
            if t[1] in LENGTH_ENDS:
                f.add(("len_end", t[1]))
            if ll[ls] > 10:
                f.add(("beyond_direct", "lit"))
            if dl[ds] > 8:
                f.add(("beyond_direct", "dist"))
    starts, ends = {}, {}
    for e in events(m):
        starts.setdefault(e[0], {})[e[1]] = e[2]
        ends.setdefault(e[0], set()).add(e[2])
        if e[0] == "match":
            n, d = e[2] - e[1], e[3]
            rel = "<" if n < d else "=" if n == d else ">"
            if d in NEAR:
                f.add(("dist", d, rel))
            if d == e[1]:
                f.add(("dist", "pos", rel))
            if d > FAR and e[1] > 32768:
                f.add(("dist", "far", rel))
    if len(m["data"]) > PIECE - 258:
        for p in PRODUCERS:
            st, en = starts.get(p, {}), ends.get(p, set())
            for k in (1, 2, 3):
                for a in AB:
                    if PIECE * k - a in st:
                        f.add(("start", p, k, a))
                for b in AB:
                    if PIECE * k + b in en:
                        f.add(("end", p, k, b))
                for a in AB:
                    for b in AB:
                        s, e = PIECE * k - a, PIECE * k + b
                        at = s
                        while at < e and at in st:
                            at = st[at]
                        if s in st and e in en and at == e if e > s else s in st and s in en:
                            f.add(("cell", p, k, a, b))
    n = len(m["data"])
    if n:
        f.add(("last_piece", n - (n - 1) // PIECE * PIECE))
    if n == 65536:
        last = events(m)[-1]
        f.add(("isize_65536_by", last[0], last[2] - last[1] if last[0] == "match" else 0))
    if m["plan"] == "tiny":
        f.add(("isize", n))
    return f


def ledger():
    """The union of every member's features."""
    if "ledger" not in _CACHE:
        out = set()
        for m in corpus():
            m["features"] = features(m)
            out |= m["features"]
        _CACHE["ledger"] = out
    return _CACHE["ledger"]


def ledger_conditions():
    """[(what, missing)]: every condition of the ledger with the tags it lacks (all empty: the corpus is what it says)."""
    L = ledger()

    def lack(tags):
        return sorted(t for t in tags if t not in L)

    split = [(a, b) for a in AB for b in AB if 0 < a + b < 3]
    conds = [
        ("every length symbol 257 .. 285", lack(("len_sym", s) for s in range(257, 286))),
        ("every distance symbol 0 .. 29", lack(("dist_sym", s) for s in range(30))),
        ("both ends of every extra-bits class of the lengths", lack(("len_end", n) for n in LENGTH_ENDS)),
        ("every code length 1 .. 15 in a literal/length code", lack(("lit_len", l) for l in range(1, 16))),
        ("every code length 1 .. 15 in a distance code", lack(("dist_len", l) for l in range(1, 16))),
        ("every code length 1 .. 7 in a code-length code", lack(("cl_len", l) for l in range(1, 8))),
        ("every longest code 1 .. 15, literal/length and distance; 1 .. 7, code-length code",
         lack([("lit_longest", l) for l in range(1, 16)] + [("dist_longest", l) for l in range(1, 16)] +
              [("cl_longest", l) for l in range(1, 8)])),
        ("codes longer than the direct tables in use, literal/length (10 bits) and distance (8 bits)",
         lack([("beyond_direct", "lit"), ("beyond_direct", "dist")])),
        ("HLIT 257 .. 286 and HDIST 1 .. 30", lack([("hlit", n) for n in range(257, 287)] + [("hdist", n) for n in range(1, 31)])),
        ("every HCLEN a valid block can have, 5 .. 19", lack(("hclen", n) for n in range(5, 20))),
        ("the incomplete sets zlib takes and no distance code", lack([("incomplete", "lit"), ("incomplete", "dist"), ("no_distance_code",)])),
        ("plain lengths, 16, 17, 18, and runs that cross into the distance lengths",
         lack([("op", o) for o in ("len", "rep16", "z17", "z18")] + [("run_crosses", o) for o in ("rep16", "z17", "z18")] +
              [("ops_mix", "plain"), ("ops_mix", "runs")])),
        ("every ordered pair of block types", lack(("pair",) + p for p in PAIRS)),
        ("every empty block, final and not", lack(("empty", t, f) for t in ("stored", "fixed", "dyn") for f in (False, True))),
        ("a block header at every bit offset", lack(("header_bit", i) for i in range(8))),
        ("every (k, a, b) cell for every producer",
         lack(("cell", p, k, a, b) for p in PRODUCERS for k in (1, 2, 3) for a in AB for b in AB if not (p == "match" and (a, b) in split))),
        ("the match cells no sequence of matches can hold, as a start and an end",
         lack([("start", "match", k, a) for k in (1, 2, 3) for a, _ in split] + [("end", "match", k, b) for k in (1, 2, 3) for _, b in split])),
        ("every named distance with length < and > (1, 2, 3: > only; 3 also =)",
         lack([("dist", d, r) for d in NEAR for r in "<=>" if not (d <= 3 and r == "<") and not (d < 3 and r == "=")])),
        ("distance = position and the far distances", lack([("dist", "pos", "<"), ("dist", "pos", ">"), ("dist", "far", "<")])),
        ("ISIZE 0 .. 9", lack(("isize", n) for n in range(10))),
        ("last pieces of 1 .. 4, 16383 and 16384 bytes", lack(("last_piece", n) for n in (1, 2, 3, 4, 16383, 16384))),
        ("ISIZE 65536 reached by a 258-byte match, a stored block and a literal",
         lack([("isize_65536_by", "match", 258), ("isize_65536_by", "stored", 0), ("isize_65536_by", "lit", 0)])),
    ]
    return conds


# ---------------------------------------------------------------------------------------------------- damaged streams
def hclen_4_stream():
    """A dynamic header with HCLEN = 4: only 16, 17, 18 and 0 have codes, so no length can be other than 0."""
    w = IC.BitWriter()
    cl = [0] * 19
    cl[0] = cl[18] = 1
    IC.dynamic_header(w, 257, 1, [("z18", 138), ("z18", 120)], cl, True, 4)
    return w.done() + b"\0\0\0\0"


def base_members():
    """The members the damage starts from: payloads of at most 1500 bytes, picked in corpus order while one adds a block type, a
    header feature or a token class that none before it had."""
    ledger()
    seen, out = set(), []
    for m in sorted(corpus(), key=lambda m: m["plan"] != "small"):  # (the tiny ones last: what only they have)
        pay = IC.split_member(m["member"])[0]
        if m["plan"] == "boundary" or len(pay) > MAX_BASE_PAYLOAD:
            continue
        new = set(t for t in m["features"] if t[0] in ("type", "pair", "empty", "incomplete", "no_distance_code", "op", "run_crosses",
                                                       "lit_longest", "dist_longest", "cl_longest", "hclen", "beyond_direct")) - seen
        if new and (len(pay) >= 8 or any(t[0] == "empty" for t in new)):
            seen |= new
            out.append(m)
    return out


def damage(members=None):
    """[{"name", "member"}]: flips, truncations, byte edits and footer edits of the base members, all seeded."""
    if members is None and "damage" in _CACHE:
        return _CACHE["damage"]
    bases = base_members() if members is None else members
    rnd = random.Random(4711)
    out = []

    def add(name, pay, crc, isize):
        out.append({"name": name, "member": IC.member(bytes(pay), crc=crc, isize=isize)})

    for m in bases:
        pay, crc, isize = IC.split_member(m["member"])
        n_bits = 8 * len(pay)

        def flipped(bits):
            p = bytearray(pay)
            for bit in bits:
                p[bit >> 3] ^= 1 << (bit & 7)
            return p

        for bit in range(min(n_bits, 48 * 8)):
            add("%s^%d" % (m["name"], bit), flipped([bit]), crc, isize)
        if n_bits > 48 * 8:
            for _ in range(200):
                bit = rnd.randrange(48 * 8, n_bits)
                add("%s^%d" % (m["name"], bit), flipped([bit]), crc, isize)
        if n_bits >= 2:
            for _ in range(50):
                bits = rnd.sample(range(n_bits), 2)
                add("%s^%d^%d" % (m["name"], bits[0], bits[1]), flipped(bits), crc, isize)
        step = max(1, len(pay) // 300)
        for cut in list(range(0, min(len(pay), 120))) + list(range(120, len(pay), step)):
            add("%s[:%d]" % (m["name"], cut), pay[:cut], crc, isize)
        for _ in range(20):
            at = rnd.randrange(len(pay) + 1)
            add("%s+byte@%d" % (m["name"], at), pay[:at] + bytes(bytearray([rnd.getrandbits(8)])) + pay[at:], crc, isize)
        if pay:
            for _ in range(20):
                at = rnd.randrange(len(pay))
                add("%s-byte@%d" % (m["name"], at), pay[:at] + pay[at + 1:], crc, isize)
        add("%s crc" % m["name"], pay, crc ^ (1 << rnd.randrange(32)), isize)
        for tag, n in (("+1", isize + 1), ("-1", isize - 1), ("+258", isize + 258), ("-258", isize - 258), ("=0", 0), ("=65536", 65536)):
            if 0 <= n <= 65536 and n != isize:
                add("%s isize%s" % (m["name"], tag), pay, crc, n)
    add("hclen_4", hclen_4_stream(), 0, 0)
    if members is None:
        _CACHE["damage"] = out
    return out


# zlib's message -> the statuses the decoder may give.  One status wherever zlib names one cause; the two symbol messages cover a code
# the tables do not hold (BAD_CODE) and a symbol that is none (286, 287; 30, 31: BAD_SYMBOL) alike.
MESSAGES = (
    ("invalid block type", (IC.BAD_BTYPE,)),
    ("invalid stored block lengths", (IC.STORED_LEN,)),
    ("invalid distance too far back", (IC.BAD_DISTANCE,)),
    ("invalid literal/length code", (IC.BAD_SYMBOL, IC.BAD_CODE)),
    ("invalid distance code", (IC.BAD_SYMBOL, IC.BAD_CODE)),
    # the header messages
    ("too many length or distance symbols", (IC.BAD_CODE,)),
    ("invalid code lengths set", (IC.BAD_CODE,)),
    ("invalid bit length repeat", (IC.BAD_CODE,)),
    ("invalid code -- missing end-of-block", (IC.BAD_CODE,)),
    ("invalid literal/lengths set", (IC.BAD_CODE,)),
    ("invalid distances set", (IC.BAD_CODE,)),
)


def _error(payload, limit=0):
    """zlib's raw inflate of the payload with the output held to `limit` bytes (0: any): (message or None, bytes, decompressobj)."""
    d = zlib.decompressobj(-15)
    try:
        return None, d.decompress(payload, limit), d
    except zlib.error as e:
        return str(e), b"", d


def verdict(payload, crc, isize):
    """What zlib says of a member: (outcome, statuses allowed, bytes or None).

    "finished": zlib reached the end of the stream with bytes D and an unused tail U.  Exactly one status: OUT_OVERRUN if len(D) >
    ISIZE, else SHORT if len(D) < ISIZE, else CRC if the CRC differs, else TRAILING if U is not empty, else OK -- and the bytes are D
    for OK, TRAILING and CRC.

    "input ran out": no error, no end of stream.  IN_OVERRUN or OUT_OVERRUN.

    "error": zlib's message names the class (MESSAGES).  The class is all there is where zlib can show that the output stayed within
    ISIZE and that the input did not end first:
      - zlib finds the error E bytes of output into the stream.  With the output held to n bytes it raises if n > E and returns n
        bytes if n < E; at n = E either may happen (it may or may not look at the next symbol with its buffer full).  So: no error
        with ISIZE + 1 bytes of room: E > ISIZE, the stream produced byte ISIZE before its error, exactly OUT_OVERRUN.  The error
        with ISIZE bytes of room (ISIZE >= 1): E <= ISIZE, the class alone.  Neither: E is ISIZE or ISIZE + 1, the class or
        OUT_OVERRUN.  zlib has no limit of 0 bytes, so with ISIZE = 0 the payload is cut before the byte at which zlib first raises:
        if what is left inflates to a byte, that byte came before the error, exactly OUT_OVERRUN; if not, the class or OUT_OVERRUN.
      - the decoder wants the 15 bits a code may have before it calls a bit pattern no code (with fewer left it says IN_OVERRUN);
        zlib says "invalid" as soon as the bits it has decide it.  If zlib raises the same message with the payload's last two bytes
        cut off, at least 16 bits stood behind the error: the class alone.  If not, IN_OVERRUN joins it."""
    msg, data, d = _error(payload)
    if msg is None:
        if not d.eof:
            return "input ran out", (IC.IN_OVERRUN, IC.OUT_OVERRUN), None
        if len(data) > isize:
            return "finished", (IC.OUT_OVERRUN,), None
        if len(data) < isize:
            return "finished", (IC.SHORT,), None
        if zlib.crc32(data) & 0xFFFFFFFF != crc:
            return "finished", (IC.CRC,), data
        return "finished", (IC.TRAILING if d.unused_data else IC.OK,), data
    allowed = None
    for text, statuses in MESSAGES:
        if text in msg:
            allowed = statuses
    assert allowed is not None, "a message of zlib's the map does not hold: %r" % msg
    if _error(payload, isize + 1)[0] is None:
        return "error", (IC.OUT_OVERRUN,), None
    if isize == 0:
        lo, hi = 0, len(payload)  # zlib raises with the first hi bytes of the payload, not with the first lo
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _error(payload[:mid])[0] is None:
                lo = mid
            else:
                hi = mid
        if _error(payload[:lo])[1]:
            return "error", (IC.OUT_OVERRUN,), None
        allowed += (IC.OUT_OVERRUN,)
    elif _error(payload, isize)[0] is None:
        allowed += (IC.OUT_OVERRUN,)
    if _error(payload[:-2])[0] != msg:
        allowed += (IC.IN_OVERRUN,)
    return "error", allowed, None


def verdicts(cases=None):
    """verdict() of every damaged stream, in order."""
    if cases is None and "verdicts" in _CACHE:
        return _CACHE["verdicts"]
    out = [verdict(*IC.split_member(c["member"])) for c in (damage() if cases is None else cases)]
    if cases is None:
        _CACHE["verdicts"] = out
    return out
