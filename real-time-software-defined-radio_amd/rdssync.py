"""RDS block synchronisation and group decoding on the host, pure Python (no GPU, no libsdr).

RdsBlockSync is the specification of the device stage (RdsSyncBank, csrc/rds_sync.hip): one
stream's differential bits D[t] -> block records (type, position, status, word).  Window p is
D[p .. p + 25], first bit first -- the link layer's convention, so positions compare with
RdsLinkBank's event positions.  Where the link layer's frame rule stops at the first damaged
block, this is what a tuner does: acquisition on two consecutive offset syndromes 26 bits apart,
a flywheel that rides over bad blocks, the (26, 16) code's burst correction and offset C'.

RdsProgramme assembles groups from those records: PI, PTY, TP, the PS name and radiotext.
"""
from __future__ import annotations

# parity matrix H (csrc/rds.hip kH, csrc/capi.hip): 26 rows of 10 bits, column 0 the most
# significant; row j belongs to the window's bit j
_H = (0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001,
      0x2DC, 0x16E, 0x0B7, 0x287, 0x39F, 0x313, 0x355, 0x376, 0x1BB, 0x201,
      0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B)

# offset syndromes, and the slot (place in the group) of each block type
SYNDROMES = {"A": 0x3D8, "B": 0x3D4, "C": 0x25C, "D": 0x258, "C'": 0x3CC}
TYPE_NAMES = ("A", "B", "C", "D", "C'")
_SYN_OF_TYPE = tuple(SYNDROMES[t] for t in TYPE_NAMES)
_TYPE_OF_SYN = {s: k for k, s in enumerate(_SYN_OF_TYPE)}
_SLOT_OF_TYPE = (0, 1, 2, 3, 2)

SEARCH, SYNC = 0, 1
_MASK26 = (1 << 26) - 1


def syndrome(window: int) -> int:
    """The 10-bit syndrome of a 26-bit window given as an integer, its first bit bit 25."""
    s = 0
    for j in range(26):
        if (window >> (25 - j)) & 1:
            s ^= _H[j]
    return s


def _half_tables():
    """syndrome(w) = lo[w & 0x1fff] ^ hi[w >> 13]"""
    lo, hi = [0] * 8192, [0] * 8192
    for v in range(1, 8192):
        b = v.bit_length() - 1                   # bit b of the low half is window bit 25 - b
        lo[v] = lo[v ^ (1 << b)] ^ _H[25 - b]
        hi[v] = hi[v ^ (1 << b)] ^ _H[12 - b]
    return lo, hi


_LO, _HI = _half_tables()


def burst_table(max_burst: int) -> dict:
    """syndrome -> error pattern (26-bit integer, first bit bit 25) for every pattern inside the
    block whose first and last flipped bits are at most max_burst - 1 apart: 26 / 51 / 99 / 191 /
    367 patterns for max_burst 1 .. 5, their syndromes distinct and non-zero."""
    if not 0 <= max_burst <= 5:
        raise ValueError(f"max_burst={max_burst} outside [0, 5]")
    table = {}
    for length in range(1, max_burst + 1):
        inner = max(length - 2, 0)
        for a in range(26 - length + 1):
            for mid in range(1 << inner):
                bits = [1] if length == 1 else [1] + [(mid >> k) & 1 for k in range(inner)] + [1]
                pat = 0
                for k, b in enumerate(bits):
                    pat |= b << (25 - a - k)
                s = syndrome(pat)
                if s == 0 or s in table:
                    raise AssertionError("burst syndromes are not distinct")
                table[s] = pat
    return table


class RdsBlockSync:
    """Block synchronisation of one stream.  process(bits) takes any number of differential bits
    (0 included) and returns the records they complete: (type, position, status, word) with type
    0 .. 3 = A .. D and 4 = C', position the index of the block's first bit since reset, status
    0 error-free / 1 corrected / 2 uncorrectable, word the 16 information bits (first bit most
    significant; as received when status is 2).  Any split of a stream into calls gives the same
    records.

    SEARCH from s0 (0 after reset): the first p with p - 26 >= s0 whose window and the window 26
    bits before it both have offset syndromes in consecutive slots gives two status-0 records and
    SYNC.  SYNC: every 26 bits the block of the expected slot, corrected through the burst table
    where its syndrome allows; in slot 2 an exact C or C' syndrome decides the type, otherwise
    the version bit (bit 11) of the B word just before it does.  bad_run counts blocks that were
    not error-free in a row (a corrected block does not feed the flywheel); at lose_after the
    block's record is still emitted and SEARCH resumes behind it."""

    def __init__(self, max_burst: int = 2, lose_after: int = 12):
        if not 1 <= lose_after <= 255:
            raise ValueError(f"lose_after={lose_after} outside [1, 255]")
        self.table = burst_table(max_burst)
        self.max_burst, self.lose_after = int(max_burst), int(lose_after)
        self.reset()

    def reset(self):
        self.nbits = 0                      # bits taken since reset
        self._w = 0                         # the last 26 bits
        self._types = [-1] * 26             # type and word of the last 26 windows, by p % 26
        self._words = [0] * 26
        self.mode, self.pos, self.slot, self.bad_run = SEARCH, 0, 0, 0    # pos: s0 / the next block
        self._b = None                      # the word of the record 26 bits back, if usable
        self.blocks = [0, 0, 0]             # cumulative: blocks of status 0 / 1 / 2
        self.acquisitions = self.losses = 0

    @property
    def synced(self) -> bool:
        return self.mode == SYNC

    def state(self) -> tuple:
        """(synced, next position, blocks of status 0, 1, 2, acquisitions, losses)"""
        return (int(self.mode == SYNC), self.pos, *self.blocks, self.acquisitions, self.losses)

    def _block(self, p, s, w):
        k = self.slot
        word = w >> 10
        if k != 2:
            typ = k
        elif s == _SYN_OF_TYPE[2]:
            typ = 2
        elif s == _SYN_OF_TYPE[4]:
            typ = 4
        elif self._b is None:
            return (2, p, 2, word)
        else:
            typ = 4 if (self._b >> 11) & 1 else 2
        e = s ^ _SYN_OF_TYPE[typ]
        if e == 0:
            return (typ, p, 0, word)
        pat = self.table.get(e)
        if pat is None:
            return (typ, p, 2, word)
        return (typ, p, 1, word ^ (pat >> 10))

    def process(self, bits) -> list:
        out = []
        for bit in bits:
            self._w = ((self._w << 1) | (int(bit) & 1)) & _MASK26
            t = self.nbits
            self.nbits += 1
            if t < 25:
                continue
            p, w = t - 25, self._w
            s = _LO[w & 0x1FFF] ^ _HI[w >> 13]
            typ = _TYPE_OF_SYN.get(s, -1)
            r = p % 26
            if self.mode == SEARCH:
                t0 = self._types[r]                                 # the window at p - 26
                if (p - 26 >= self.pos and typ >= 0 and t0 >= 0
                        and _SLOT_OF_TYPE[typ] == (_SLOT_OF_TYPE[t0] + 1) & 3):
                    out.append((t0, p - 26, 0, self._words[r]))
                    out.append((typ, p, 0, w >> 10))
                    self.blocks[0] += 2
                    self.acquisitions += 1
                    self.mode, self.pos, self.slot, self.bad_run = SYNC, p + 26, (_SLOT_OF_TYPE[typ] + 1) & 3, 0
                    self._b = w >> 10
            elif p == self.pos:
                rec = self._block(p, s, w)
                out.append(rec)
                self.blocks[rec[2]] += 1
                self._b = rec[3] if rec[2] <= 1 else None
                self.bad_run = 0 if rec[2] == 0 else self.bad_run + 1
                self.pos, self.slot = p + 26, (self.slot + 1) & 3
                if self.bad_run >= self.lose_after:
                    self.losses += 1
                    self.mode, self.bad_run, self._b = SEARCH, 0, None
            self._types[r], self._words[r] = typ, w >> 10
        return out


def _char(v: int) -> str:
    return chr(v) if 0x20 <= v <= 0x7E else "?"


class RdsProgramme:
    """One station's programme data from its block records.  feed(records) takes the 4-tuples of
    RdsBlockSync.process / RdsSyncBank.blocks() in order and decodes every group it finds: an A,
    B, C or C', D run 26 bits apart, all of status <= 1.

    pi: block A's word, or block C' of a version-B group.  pty, tp: from block B.  ps: the
    eight-character name from groups 0A / 0B (segment b & 3, two characters of block D);
    ps_complete once all four segments were seen since the last PI change.  radiotext: groups 2A
    (four characters of C and D at 4 (b & 15)) and 2B (two of D at 2 (b & 15)); a change of the
    text A/B flag (bit 4) clears it and 0x0D ends it.  Bytes 0x20 .. 0x7E are ASCII, the rest
    '?'; a place not yet received reads as a blank."""

    def __init__(self):
        self.pi = self.pty = self.tp = None
        self.groups = 0
        self._run = []
        self._clear()

    def _clear(self):
        self._ps = [" "] * 8
        self._ps_seen = set()
        self._rt = [None] * 64
        self._rt_flag = None

    @property
    def ps(self) -> str:
        return "".join(self._ps)

    @property
    def ps_complete(self) -> bool:
        return len(self._ps_seen) == 4

    @property
    def radiotext(self) -> str:
        out = []
        for v in self._rt:
            if v == 0x0D:
                break
            out.append(" " if v is None else _char(v))
        return "".join(out).rstrip(" ")

    def feed(self, records):
        for typ, pos, status, word in records:
            typ, pos, word = int(typ), int(pos), int(word)
            slot = _SLOT_OF_TYPE[typ]
            if status > 1:
                self._run = []
                continue
            if self._run and not (slot == len(self._run) and pos == self._run[-1][1] + 26):
                self._run = []
            if slot == len(self._run):
                self._run.append((typ, pos, word))
            if len(self._run) == 4:
                self._group(*[(t, w) for t, _, w in self._run])
                self._run = []

    def _group(self, a, b, c, d):
        bw = b[1]
        version_b = (bw >> 11) & 1
        if version_b != (c[0] == 4):
            return
        pi = c[1] if version_b else a[1]
        if pi != self.pi:
            self.pi = pi
            self._clear()
        self.groups += 1
        self.tp, self.pty = (bw >> 10) & 1, (bw >> 5) & 31
        gtype = bw >> 12
        if gtype == 0:
            seg = bw & 3
            self._ps[2 * seg:2 * seg + 2] = [_char(d[1] >> 8), _char(d[1] & 0xFF)]
            self._ps_seen.add(seg)
        elif gtype == 2:
            flag = (bw >> 4) & 1
            if self._rt_flag is not None and flag != self._rt_flag:
                self._rt = [None] * 64
            self._rt_flag = flag
            seg = bw & 15
            if version_b:
                self._rt[2 * seg:2 * seg + 2] = [d[1] >> 8, d[1] & 0xFF]
            else:
                self._rt[4 * seg:4 * seg + 4] = [c[1] >> 8, c[1] & 0xFF, d[1] >> 8, d[1] & 0xFF]
