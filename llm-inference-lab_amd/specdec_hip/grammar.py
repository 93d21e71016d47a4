"""Token automata for grammar-constrained decoding (host side; pure Python + numpy).

A TokenFSM is the table the device walks (csrc/grammar.hip, the contract is at sd_logit_process_fsm in include/specdec_hip.h):
`next` uint16 [S][V], next[s][v] = the state after token v in state s, 0xFFFF = v is not allowed in s. It is compiled here from
a regular expression over the BYTES of the tokens (from_regex), from a closed list of answers (from_choices), or merged from
several automata so that the rows of one batch carry different grammars (union).

Invariant (check()): every state reachable from `start` allows at least one token; a state that allows `eos_id` (an accepting
state) sends it to a terminal state that allows only `eos_id`, to itself; and only live transitions are kept — transitions
into states from which an accepting state can still be reached — so a decoder that follows allowed() can always finish.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

NONE = 0xFFFF          # table entry: the token is not allowed in the state
DEAD = 0xFFFF          # a row's state after a token its automaton did not allow: only eos is allowed, DEAD stays DEAD
UNCONSTRAINED = -1     # a row's state: no grammar
MAX_STATES = 65534
DEFAULT_MAX_TABLE_BYTES = 2 << 30


def _check_size(S: int, V: int, max_table_bytes: int) -> None:
    if S > MAX_STATES:
        raise ValueError(f"token automaton has {S} states; the table's uint16 entries hold at most {MAX_STATES}")
    nbytes = S * V * 2
    if nbytes > max_table_bytes:
        raise ValueError(f"token automaton table is {nbytes} bytes ({S} states x {V} tokens x 2), above max_table_bytes = {max_table_bytes}")


class TokenFSM:
    """next: uint16 [S][V]; start: the state of a fresh row; eos_id: the token accepting states allow and that ends the output."""

    def __init__(self, next: np.ndarray, start: int, eos_id: int):
        next = np.ascontiguousarray(next, dtype=np.uint16)
        if next.ndim != 2 or not 1 <= next.shape[0] <= MAX_STATES:
            raise ValueError(f"TokenFSM: next must be uint16 [S][V] with 1 <= S <= {MAX_STATES}, got {next.shape}")
        if not 0 <= int(eos_id) < next.shape[1]:
            raise ValueError(f"TokenFSM: eos_id {eos_id} outside [0, {next.shape[1]})")
        if not 0 <= int(start) < next.shape[0]:
            raise ValueError(f"TokenFSM: start {start} outside [0, {next.shape[0]})")
        self.next, self.start, self.eos_id = next, int(start), int(eos_id)

    @property
    def S(self) -> int:
        return int(self.next.shape[0])

    @property
    def V(self) -> int:
        return int(self.next.shape[1])

    # ---- the host's in-order view
    def step(self, state: int, token: int) -> int:
        state = int(state)
        if state < 0:
            return UNCONSTRAINED
        if state >= self.S or not 0 <= int(token) < self.V:
            return DEAD
        nx = int(self.next[state, int(token)])
        return DEAD if nx >= self.S else nx

    def walk(self, state: int, tokens: Sequence[int]) -> int:
        for t in tokens:
            state = self.step(state, t)
        return DEAD if int(state) >= self.S else int(state)

    def allowed(self, state: int) -> np.ndarray:
        """the ids allowed in `state`, ascending (every id for an unconstrained row, eos alone in DEAD)"""
        state = int(state)
        if state < 0:
            return np.arange(self.V)
        if state >= self.S:
            return np.array([self.eos_id])
        return np.flatnonzero(self.next[state] != NONE)

    def accepts(self, tokens: Sequence[int], state: Optional[int] = None) -> bool:
        """`tokens` lead from `state` (default: start) to a state that allows eos"""
        s = self.walk(self.start if state is None else state, tokens)
        return s < self.S and self.next[s, self.eos_id] != NONE

    # ---- the invariant
    def _edges(self) -> List[np.ndarray]:
        return [np.unique(row[row != NONE]).astype(np.int64) for row in self.next]

    def _reachable(self, starts: Sequence[int], edges: List[np.ndarray]) -> np.ndarray:
        seen = np.zeros(self.S, dtype=bool)
        todo = [int(s) for s in starts]
        for s in todo:
            seen[s] = True
        while todo:
            for t in edges[todo.pop()]:
                if not seen[t]:
                    seen[t] = True
                    todo.append(int(t))
        return seen

    def _live(self, edges: List[np.ndarray]) -> np.ndarray:
        """states from which a terminal state (one that allows eos to itself) can be reached"""
        S, e = self.S, self.eos_id
        live = np.array([self.next[s, e] == s for s in range(S)])
        changed = True
        while changed:
            changed = False
            for s in range(S):
                if not live[s] and len(edges[s]) and live[edges[s]].any():
                    live[s] = changed = True
        return live

    def check(self, starts: Optional[Sequence[int]] = None) -> "TokenFSM":
        S, V, e = self.S, self.V, self.eos_id
        bad = (self.next != NONE) & (self.next >= S)
        if bad.any():
            raise ValueError(f"TokenFSM.check: entry {int(self.next[bad][0])} is neither a state below {S} nor 0xFFFF")
        edges = self._edges()
        reach = self._reachable([self.start] if starts is None else starts, edges)
        live = self._live(edges)
        for s in np.flatnonzero(reach):
            row = self.next[s]
            if not (row != NONE).any():
                raise ValueError(f"TokenFSM.check: state {s} allows no token")
            if row[e] != NONE:
                t = int(row[e])
                trow = self.next[t]
                if trow[e] != t or int((trow != NONE).sum()) != 1:
                    raise ValueError(f"TokenFSM.check: eos in state {s} leads to state {t}, which is not a terminal state (eos only, to itself)")
            if not live[edges[s]].all():
                raise ValueError(f"TokenFSM.check: state {s} keeps a transition into a state from which no accepting state can be reached")
        return self

    def _pruned(self) -> "TokenFSM":
        """drop transitions into states that cannot reach a terminal state, then the states `start` no longer reaches"""
        edges = self._edges()
        live = self._live(edges)
        if not live[self.start]:
            raise ValueError("the grammar accepts nothing that this vocabulary can spell")
        nxt = self.next.copy()
        dead_target = np.zeros(NONE + 1, dtype=bool)
        dead_target[:self.S] = ~live
        nxt[dead_target[nxt]] = NONE
        t = TokenFSM(nxt, self.start, self.eos_id)
        keep = np.flatnonzero(t._reachable([t.start], t._edges()))
        remap = np.full(NONE + 1, NONE, dtype=np.uint16)
        remap[keep] = np.arange(len(keep), dtype=np.uint16)
        return TokenFSM(remap[nxt[keep]], int(remap[self.start]), self.eos_id)

    # ---- constructors
    @classmethod
    def from_choices(cls, choices: Sequence[Sequence[int]], V: int, eos_id: int,
                     max_table_bytes: int = DEFAULT_MAX_TABLE_BYTES) -> "TokenFSM":
        """A trie: the output is exactly one of the token sequences, then eos."""
        choices = [[int(t) for t in c] for c in choices]
        if not choices:
            raise ValueError("from_choices: no sequences")
        for c in choices:
            if any(not 0 <= t < V for t in c) or eos_id in c:
                raise ValueError(f"from_choices: sequence {c} holds an id outside [0, {V}) or the eos id")
        nodes: List[dict] = [{}]
        accept = [False]
        for c in choices:
            s = 0
            for t in c:
                if t not in nodes[s]:
                    nodes[s][t] = len(nodes)
                    nodes.append({})
                    accept.append(False)
                s = nodes[s][t]
            accept[s] = True
        S = len(nodes) + 1
        _check_size(S, V, max_table_bytes)
        nxt = np.full((S, V), NONE, dtype=np.uint16)
        for s, kids in enumerate(nodes):
            for t, d in kids.items():
                nxt[s, t] = d
            if accept[s]:
                nxt[s, eos_id] = S - 1
        nxt[S - 1, eos_id] = S - 1
        return cls(nxt, 0, eos_id).check()

    @classmethod
    def from_regex(cls, pattern: str, vocab_bytes: Sequence[Optional[bytes]], eos_id: int,
                   max_table_bytes: int = DEFAULT_MAX_TABLE_BYTES) -> "TokenFSM":
        """Full-match semantics over the bytes of the tokens: a token sequence is accepted iff the concatenation of its tokens'
        bytes matches `pattern` as a whole. vocab_bytes[id] = the token's bytes, None (or empty) = never allowed.

        Supported: literals and escapes (\\d \\w \\s \\D \\W \\S \\n \\t \\r \\f \\v \\xHH and escaped punctuation), `.` (any byte
        but a newline), classes and negated classes with ranges, groups (also `(?:...)`), `|`, and `* + ? {m} {m,} {m,n}`.
        Anything else raises ValueError naming the construct."""
        V = len(vocab_bytes)
        if not 0 <= int(eos_id) < V:
            raise ValueError(f"from_regex: eos_id {eos_id} outside [0, {V})")
        trans, accept = _byte_dfa(pattern)           # [Sb][256] int32, -1 = no transition; state 0 = start
        Sb = trans.shape[0]
        S = Sb + 1
        _check_size(S, V, max_table_bytes)
        # token DFA: all V tokens advance together, one byte position at a time; row Sb of `tr` is the sink
        tr = np.vstack([np.where(trans < 0, Sb, trans), np.full((1, 256), Sb, dtype=trans.dtype)]).astype(np.int32)
        lens = np.array([len(b) if b is not None else 0 for b in vocab_bytes], dtype=np.int64)
        lens[eos_id] = 0
        L = int(lens.max()) if V else 0
        tb = np.zeros((V, max(L, 1)), dtype=np.uint8)
        for v, b in enumerate(vocab_bytes):
            if lens[v]:
                tb[v, :lens[v]] = np.frombuffer(b, dtype=np.uint8)
        nxt = np.full((S, V), NONE, dtype=np.uint16)
        valid = np.flatnonzero(lens > 0)
        order = valid[np.argsort(lens[valid], kind="stable")[::-1]]   # longest first: the tokens still advancing at position p are a prefix
        sl = lens[order]
        rows_per = max(1, (64 << 20) // max(1, 4 * len(order)))        # states per chunk: the working grid stays below 64 MiB
        for s0 in range(0, Sb, rows_per):
            s1 = min(Sb, s0 + rows_per)
            cur = np.repeat(np.arange(s0, s1, dtype=np.int32)[:, None], len(order), axis=1)
            for p in range(L):
                n = int(np.searchsorted(-sl, -p, side="left"))        # tokens longer than p
                if n == 0:
                    break
                cur[:, :n] = tr[cur[:, :n], tb[order[:n], p][None, :]]
            out = np.where(cur == Sb, NONE, cur).astype(np.uint16)
            nxt[s0:s1, order] = out
        nxt[:Sb, eos_id] = np.where(accept, Sb, NONE).astype(np.uint16)
        nxt[Sb, eos_id] = Sb
        return cls(nxt, 0, eos_id)._pruned().check()

    @staticmethod
    def union(fsms: Sequence["TokenFSM"], max_table_bytes: int = DEFAULT_MAX_TABLE_BYTES) -> Tuple["TokenFSM", List[int]]:
        """One table holding every member at a state offset -> (the table, each member's start state in it). The merged
        automaton's own `start` is the first member's."""
        fsms = list(fsms)
        if not fsms:
            raise ValueError("union: no automata")
        V, e = fsms[0].V, fsms[0].eos_id
        if any(f.V != V or f.eos_id != e for f in fsms):
            raise ValueError("union: the automata differ in vocabulary size or eos id")
        S = sum(f.S for f in fsms)
        _check_size(S, V, max_table_bytes)
        nxt = np.empty((S, V), dtype=np.uint16)
        starts, off = [], 0
        for f in fsms:
            nxt[off:off + f.S] = np.where(f.next == NONE, NONE, f.next.astype(np.int64) + off).astype(np.uint16)
            starts.append(off + f.start)
            off += f.S
        return TokenFSM(nxt, starts[0], e), starts


def from_tokenizer(pattern: str, tokenizer, V: int, eos_id: Optional[int] = None,
                   max_table_bytes: int = DEFAULT_MAX_TABLE_BYTES) -> TokenFSM:
    """from_regex with vocab_bytes[id] = tokenizer.decode([id]).encode("utf-8") for id < V.

    Limitation: ids whose decoded text contains U+FFFD, and special ids, are never allowed. A byte-level BPE vocabulary spells
    some characters with several tokens that are each only part of a UTF-8 sequence; decoded alone they give U+FFFD, so text
    that needs them (most non-Latin scripts, emoji) cannot be produced under such a grammar. ASCII patterns are not affected."""
    if eos_id is None:
        eos_id = getattr(tokenizer, "eos_token_id", None)
        if eos_id is None:
            raise ValueError("from_tokenizer: the tokenizer names no eos token; pass eos_id")
    special = set(int(i) for i in (getattr(tokenizer, "all_special_ids", None) or []))
    vocab: List[Optional[bytes]] = []
    for i in range(int(V)):
        if i in special:
            vocab.append(None)
            continue
        try:
            text = tokenizer.decode([i])
        except Exception:
            text = None
        vocab.append(None if not text or "\ufffd" in text else text.encode("utf-8"))
    return TokenFSM.from_regex(pattern, vocab, int(eos_id), max_table_bytes)


TokenFSM.from_tokenizer = staticmethod(from_tokenizer)


# ---- regular expression -> byte DFA ------------------------------------------------------------------------------------------
_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ALL = frozenset(range(256))
_CLASS_ESC = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _ALL - _DIGIT, "W": _ALL - _WORD, "S": _ALL - _SPACE}
_CHAR_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0, "a": 7}
_MAX_REPEAT = 1000


class _Parser:
    """pattern -> AST: ("set", frozenset of bytes) | ("cat", [..]) | ("alt", [..]) | ("rep", node, lo, hi or None)"""

    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("from_regex: the pattern must be a str")
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"from_regex: unsupported construct {what} at position {self.i} of {self.p!r}")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "?":
                lo, hi = 0, 1
            elif c == "{":
                j = self.p.find("}", self.i)
                body = self.p[self.i + 1:j] if j > 0 else ""
                parts = body.split(",")
                if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()):
                    self.fail("'{' that is not a repeat count {m}, {m,} or {m,n}")
                lo = int(parts[0])
                hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
                if (hi is not None and hi < lo) or max(lo, hi or 0) > _MAX_REPEAT:
                    self.fail(f"repeat count {{{body}}}")
                self.i = j
            else:
                return node
            self.i += 1
            if self.peek() in ("?", "+"):
                self.fail(f"lazy or possessive quantifier '{self.peek()}' after a quantifier")
            node = ("rep", node, lo, hi)

    def escape(self, in_class: bool):
        """after a backslash -> frozenset of bytes"""
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        if c in _CLASS_ESC:
            return _CLASS_ESC[c]
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                self.fail("\\x without two hex digits")
            self.i += 2
            return frozenset([int(h, 16)])
        if c == "b" and in_class:
            return frozenset([8])
        if c in _CHAR_ESC:
            return frozenset([_CHAR_ESC[c]])
        if c.isdigit():
            self.fail(f"backreference \\{c}")
        if c.isalnum():
            self.fail(f"escape \\{c}" + (" (anchors and word boundaries are not supported)" if c in "bBAZz" else ""))
        if ord(c) > 127:
            self.fail("escaped non-ASCII character")
        return frozenset([ord(c)])

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] == "?:":
                    self.i += 2
                else:
                    self.fail(f"group extension '({self.p[self.i:self.i + 3]}' (lookaround, named groups and flags are not supported)")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            self.i += 1
            return ("set", _ALL - {10})
        if c == "\\":
            self.i += 1
            return ("set", self.escape(False))
        if c in ("^", "$"):
            self.fail(f"anchor '{c}' (the whole output is matched: full-match semantics)")
        if c in ("*", "+", "?", "{"):
            self.fail(f"quantifier '{c}' with nothing to repeat")
        self.i += 1
        bs = c.encode("utf-8")
        if len(bs) == 1:
            return ("set", frozenset(bs))
        return ("cat", [("set", frozenset([b])) for b in bs])

    def klass(self):
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        members = set()
        first = True
        while True:
            c = self.peek()
            if c == "":
                self.fail("unterminated '['")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i:self.i + 2] in ("[:", "[=", "[."):
                self.fail("POSIX class inside '[...]'")
            lo = self.class_item()
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_item()
                if len(lo) != 1 or len(hi) != 1 or min(hi) < min(lo):
                    self.fail("bad range in '[...]'")
                members.update(range(min(lo), min(hi) + 1))
            else:
                members.update(lo)
        s = frozenset(members)
        return ("set", _ALL - s if neg else s)

    def class_item(self):
        c = self.peek()
        self.i += 1
        if c == "\\":
            return self.escape(True)
        if ord(c) > 127:
            self.fail("non-ASCII character inside '[...]' (classes are over single bytes)")
        return frozenset([ord(c)])


class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[frozenset, int]]] = []

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """Thompson construction -> (entry, exit)"""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            if node[1]:
                self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if hi is None:
            x, y = self.build(sub)
            loop = self.new()
            self.eps[b].append(loop)
            self.eps[loop].append(x)
            self.eps[y].append(loop)
            b = loop
        else:
            end = self.new()
            for _ in range(hi - lo):
                x, y = self.build(sub)
                self.eps[b].append(end)
                self.eps[b].append(x)
                b = y
            self.eps[b].append(end)
            b = end
        return a, b

    def closure(self, states) -> frozenset:
        seen = set(states)
        todo = list(states)
        while todo:
            for t in self.eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)


def _byte_dfa(pattern: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (trans int32 [S][256] with -1 = no transition, accept bool [S]); state 0 is the start; trimmed (every state reaches
    an accepting one) and minimised (Moore's refinement)."""
    nfa = _NFA()
    entry, final = nfa.build(_Parser(pattern).parse())
    if len(nfa.eps) > 200000:
        raise ValueError(f"from_regex: the pattern expands to {len(nfa.eps)} NFA states")
    # bytes that every set of the pattern treats alike form one class: the subset construction runs over classes
    sets = list({bs for es in nfa.edges for bs, _ in es})
    sig = np.zeros((256, max(len(sets), 1)), dtype=bool)
    for k, bs in enumerate(sets):
        sig[list(bs), k] = True
    _, rep, cls_of = np.unique(sig, axis=0, return_index=True, return_inverse=True)
    cls_of = np.asarray(cls_of).reshape(-1)
    start = nfa.closure([entry])
    index = {start: 0}
    order = [start]
    rows: List[List[int]] = []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = []
        for r in rep:
            tgt = {t for s in cur for bs, t in nfa.edges[s] if int(r) in bs}
            if not tgt:
                row.append(-1)
                continue
            c = nfa.closure(tgt)
            if c not in index:
                index[c] = len(order)
                order.append(c)
                if len(order) > MAX_STATES:
                    raise ValueError(f"from_regex: the pattern needs more than {MAX_STATES} DFA states")
            row.append(index[c])
        rows.append(row)
    ctrans = np.array(rows, dtype=np.int64).reshape(len(order), len(rep))
    accept = np.array([final in c for c in order])
    # trim: states that reach no accepting state go (transitions into them become -1)
    n = len(order)
    live = accept.copy()
    while True:
        t = np.where(ctrans >= 0, live[np.maximum(ctrans, 0)], False).any(axis=1) | live
        if (t == live).all():
            break
        live = t
    if not live[0]:
        raise ValueError(f"from_regex: {pattern!r} matches nothing")
    ctrans = np.where((ctrans >= 0) & live[np.maximum(ctrans, 0)], ctrans, -1)
    # Moore: refine {accepting, not} by the classes' successors until stable; dead rows (not live) never appear as targets
    label = np.where(live, accept.astype(np.int64) + 1, 0)
    while True:
        succ = np.where(ctrans >= 0, label[np.maximum(ctrans, 0)], -1)
        _, new = np.unique(np.column_stack([label, succ]), axis=0, return_inverse=True)
        new = np.asarray(new).reshape(-1)
        if len(np.unique(new)) == len(np.unique(label)):
            break
        label = new
    label = new
    # renumber: start first, then by first appearance among live states
    ids = {}
    for s in [0] + [s for s in range(n) if live[s]]:
        ids.setdefault(int(label[s]), len(ids))
    S = len(ids)
    trans = np.full((S, 256), -1, dtype=np.int32)
    acc = np.zeros(S, dtype=bool)
    for s in range(n):
        if not live[s]:
            continue
        d = ids[int(label[s])]
        acc[d] = accept[s]
        row = ctrans[s]
        mapped = np.array([ids[int(label[t])] if t >= 0 else -1 for t in row], dtype=np.int32)
        trans[d] = mapped[cls_of]
    return trans, acc
