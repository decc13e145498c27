"""Grammars for CTC grammar decoding (``dsmi_grammar``): a small syntax compiled to the token graph the kernel searches.

    $digit = nul | en | to | tre ;
    (tænd | sluk) lyset [i (stuen | køkkenet:-0.5)] $digit*

Words are runs of label characters.  Juxtaposition is sequence, ``|`` alternatives, ``( )`` grouping, ``[ ]`` optional, postfix
``*`` any number of times and ``+`` at least once.  Rules ``$name = ... ;`` come before the main expression; a ``$name``
reference expands in line (recursion is an error).  ``word:-1.5`` puts a weight (a natural-log score, added once) on the word's
first character.  Text is normalised as transcripts are: lower case, whitespace runs to one space.

The graph is the position automaton (Glushkov) of the expression over characters: one node per character occurrence and no
epsilon arcs, so ``first`` gives the start flags, ``last`` the final flags, ``follow`` the arcs and nullable gives ``empty_ok``.
Every word carries a leading space node; a sentence's first word is entered at its first character instead.  Then nodes with
equal label, weight, start flag and predecessor set are merged until nothing changes (the same strings reach both, so the
language stays): a loop over W words becomes one shared space node and a prefix trie, about 5 W nodes and 6 W arcs and not
W * W arcs.  Host only: numpy, no torch.
"""
import re

import numpy as np

MAX_NODES = 2048        # DSMI_GRAMMAR_MAX_NODES
MAX_ARCS = 8192         # DSMI_GRAMMAR_MAX_ARCS
START, FINAL = 1, 2     # DSMI_GRAMMAR_START, DSMI_GRAMMAR_FINAL

_OPERATORS = "|()[]*+;=$:"
_NUMBER = re.compile(r"[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?")
_NAME = re.compile(r"[A-Za-z0-9_]+")


def normalise(text):
    return " ".join(text.lower().split())


class Grammar:
    """The compiled graph: ``labels`` int32 [N], ``weights`` float32 [N], ``flags`` int32 [N] (START | FINAL), ``arc_off`` int32
    [N + 1] and ``arc_pred`` int32 (CSR: the predecessors of each node, ascending), ``empty_ok``; ``alphabet`` is the label
    string or list it was compiled for."""

    def __init__(self, text, labels, blank_index=0, _merge=True, _limits=True):
        self.alphabet = labels
        self.blank = blank_index
        self._ids = {c: i for i, c in enumerate(labels) if i != blank_index}
        if " " not in self._ids:
            raise ValueError("grammar: the labels have no space")
        rules, main = _parse(_tokens(text, self._ids))
        self._compile(rules, main, _merge, _limits)

    @classmethod
    def from_sentences(cls, sentences, labels, blank_index=0, _merge=True, _limits=True):
        """The grammar that accepts exactly these sentences (normalised; an empty one makes the empty sentence acceptable)."""
        self = cls.__new__(cls)
        self.alphabet = labels
        self.blank = blank_index
        self._ids = {c: i for i, c in enumerate(labels) if i != blank_index}
        if " " not in self._ids:
            raise ValueError("grammar: the labels have no space")
        alts = []
        for s in sentences:
            words = normalise(s).split()
            for w in words:
                for c in w:
                    if c not in self._ids:
                        raise ValueError("grammar: character %r of %r is not a label" % (c, s))
            alts.append(("seq", [("word", w, 0.0) for w in words]))
        if not alts:
            raise ValueError("grammar: no sentence")
        self._compile({}, ("alt", alts), _merge, _limits)
        return self

    # ---- expression -> position automaton -> merged graph
    def _compile(self, rules, main, merge, limits=True):
        lab, wt, follow = [], [], []
        first_char = {}                  # a word's space node -> its first character's node

        def word(w, weight):
            base = len(lab)
            lab.append(self._ids[" "]); wt.append(0.0); follow.append(set())
            for k, c in enumerate(w):
                lab.append(self._ids[c]); wt.append(float(weight) if k == 0 else 0.0); follow.append(set())
                follow[base + k].add(base + k + 1)
            first_char[base] = base + 1
            return False, {base}, {base + len(w)}

        def build(e, stack):
            kind = e[0]
            if kind == "word":
                return word(e[1], e[2])
            if kind == "ref":
                if e[1] in stack:
                    raise ValueError("grammar: rule $%s is recursive" % e[1])
                if e[1] not in rules:
                    raise ValueError("grammar: rule $%s is not defined" % e[1])
                return build(rules[e[1]], stack + (e[1],))
            if kind == "seq":
                nullable, first, last = True, set(), set()
                for x in e[1]:
                    n2, f2, l2 = build(x, stack)
                    for p in last:
                        follow[p] |= f2
                    if nullable:
                        first |= f2
                    last = l2 | last if n2 else l2
                    nullable = nullable and n2
                return nullable, first, last
            if kind == "alt":
                nullable, first, last = False, set(), set()
                for x in e[1]:
                    n2, f2, l2 = build(x, stack)
                    nullable, first, last = nullable or n2, first | f2, last | l2
                return nullable, first, last
            n2, f2, l2 = build(e[1], stack)
            if kind in ("star", "plus"):
                for p in l2:
                    follow[p] |= f2
            return (n2 if kind == "plus" else True), f2, l2

        nullable, first, last = build(main, ())
        N = len(lab)
        start = [False] * N
        for p in first:
            start[first_char.get(p, p)] = True
        final = [p in last for p in range(N)]
        preds = [set() for _ in range(N)]
        for p in range(N):
            for q in follow[p]:
                preds[q].add(p)
        # ---- merge to a fixpoint: equal label, weight, start flag and predecessor set
        rep = list(range(N))
        while merge:
            seen, changed = {}, False
            for p in range(N):
                if rep[p] != p:
                    continue
                key = (lab[p], wt[p], start[p], frozenset(preds[p]))
                q = seen.setdefault(key, p)
                if q != p:
                    rep[p] = q
                    final[q] = final[q] or final[p]
                    changed = True
            if not changed:
                break
            rep = [rep[rep[p]] for p in range(N)]
            for p in range(N):
                if rep[p] == p:
                    preds[p] = {rep[q] for q in preds[p]}
        # ---- what a start node reaches, renumbered in the order of the positions
        succ = [[] for _ in range(N)]
        for p in range(N):
            if rep[p] == p:
                for q in preds[p]:
                    succ[q].append(p)
        reach, todo = set(), [p for p in range(N) if rep[p] == p and start[p]]
        while todo:
            p = todo.pop()
            if p not in reach:
                reach.add(p)
                todo.extend(succ[p])
        keep = sorted(reach)
        new = {p: i for i, p in enumerate(keep)}
        rows = [sorted(new[q] for q in preds[p] if q in new) for p in keep]
        n_arcs = sum(len(r) for r in rows)
        if limits and len(keep) > MAX_NODES:
            raise ValueError("grammar: %d nodes, more than the limit of %d" % (len(keep), MAX_NODES))
        if limits and n_arcs > MAX_ARCS:
            raise ValueError("grammar: %d arcs, more than the limit of %d" % (n_arcs, MAX_ARCS))
        self.labels = np.array([lab[p] for p in keep], dtype=np.int32)
        self.weights = np.array([wt[p] for p in keep], dtype=np.float32)
        self.flags = np.array([(START if start[p] else 0) | (FINAL if final[p] else 0) for p in keep], dtype=np.int32)
        self.arc_off = np.zeros(len(keep) + 1, dtype=np.int32)
        self.arc_off[1:] = np.cumsum([len(r) for r in rows])
        self.arc_pred = np.array([q for r in rows for q in r], dtype=np.int32)
        self.empty_ok = bool(nullable)

    n_nodes = property(lambda self: len(self.labels))
    n_arcs = property(lambda self: len(self.arc_pred))

    def preds(self, n):
        return self.arc_pred[self.arc_off[n]:self.arc_off[n + 1]]

    def text_of(self, nodes):
        """The text of a path of node ids."""
        return "".join(self.alphabet[self.labels[n]] for n in nodes)

    # ---- plain host code over the graph, for users and tests
    def _step(self, cur, label):
        """The nodes with ``label`` entered from the node set ``cur`` (None: from the start)."""
        out = set()
        for n in np.nonzero(self.labels == label)[0]:
            if (cur is None and self.flags[n] & START) or (cur is not None and any(p in cur for p in self.preds(n))):
                out.add(int(n))
        return out

    def accepts(self, text):
        text = normalise(text)
        if not text:
            return self.empty_ok
        cur = None
        for c in text:
            if c not in self._ids:
                return False
            cur = self._step(cur, self._ids[c])
            if not cur:
                return False
        return any(self.flags[n] & FINAL for n in cur)

    def weight_of(self, text):
        """The weight the graph gives a sentence, as ``dsmi_grammar_posterior`` counts it: the log-sum-exp, over the node paths
        that spell the (normalised) text, of the sum of their nodes' weights -- 0.0 for one path without weights, ln 2 for two --
        or None when the grammar does not accept it."""
        text = normalise(text)
        if not text:
            return 0.0 if self.empty_ok else None
        w = self.weights.astype(np.float64)
        cur = None                       # node -> the log-sum over the paths that end in it
        for c in text:
            if c not in self._ids:
                return None
            nxt = {}
            for n in np.nonzero(self.labels == self._ids[c])[0]:
                n = int(n)
                if cur is None:
                    if self.flags[n] & START:
                        nxt[n] = w[n]
                else:
                    inn = [cur[int(p)] for p in self.preds(n) if int(p) in cur]
                    if inn:
                        nxt[n] = float(np.logaddexp.reduce(inn)) + w[n]
            if not nxt:
                return None
            cur = nxt
        ends = [v for n, v in cur.items() if self.flags[n] & FINAL]
        return float(np.logaddexp.reduce(ends)) if ends else None

    def sentences(self, max_count=1000):
        """The accepted sentences, shortest first and in label order among equals, at most ``max_count`` of them."""
        out = [""] if self.empty_ok else []
        front = {(): None}
        by_label = sorted(set(int(v) for v in self.labels))
        while front and len(out) < max_count:
            nxt = {}
            for s in sorted(front):
                for c in by_label:
                    cur = self._step(front[s], c)
                    if cur:
                        nxt[s + (c,)] = cur
            for s in sorted(nxt):
                if len(out) < max_count and any(self.flags[n] & FINAL for n in nxt[s]):
                    out.append("".join(self.alphabet[c] for c in s))
            front = nxt
        return out


def _tokens(text, ids):
    """(kind, value) pairs: ('op', c), ('word', str), ('ref', name), ('num', float)."""
    text = normalise(text)
    out, i = [], 0
    while i < len(text):
        c = text[i]
        if c == " ":
            i += 1
        elif c == "$":
            m = _NAME.match(text, i + 1)
            if not m:
                raise ValueError("grammar: a name must follow $ (at %d)" % i)
            out.append(("ref", m.group(0)))
            i = m.end()
        elif c == ":":
            m = _NUMBER.match(text, i + 1)
            if not m or not out or out[-1][0] != "word":
                raise ValueError("grammar: ':' takes a number and follows a word (at %d)" % i)
            value = float(m.group(0))
            if not abs(value) <= float(np.finfo(np.float32).max):
                raise ValueError("grammar: weight %s is not finite" % m.group(0))
            out.append(("num", value))
            i = m.end()
        elif c in _OPERATORS:
            out.append(("op", c))
            i += 1
        else:
            j = i
            while j < len(text) and text[j] != " " and text[j] not in _OPERATORS:
                if text[j] not in ids:
                    raise ValueError("grammar: character %r is not a label (at %d)" % (text[j], j))
                j += 1
            out.append(("word", text[i:j]))
            i = j
    return out


def _parse(toks):
    """The rules {name: expression} and the main expression.  alt := seq ('|' seq)*; seq := item*; item := atom ('*' | '+')*;
    atom := word [':' number] | $name | '(' alt ')' | '[' alt ']'."""
    pos = [0]

    def peek():
        return toks[pos[0]] if pos[0] < len(toks) else (None, None)

    def take():
        pos[0] += 1
        return toks[pos[0] - 1]

    def alt():
        items = [seq()]
        while peek() == ("op", "|"):
            take()
            items.append(seq())
        return items[0] if len(items) == 1 else ("alt", items)

    def seq():
        items = []
        while peek()[0] in ("word", "ref") or peek() in (("op", "("), ("op", "[")):
            items.append(item())
        if not items:
            raise ValueError("grammar: an expression is empty (at token %d)" % pos[0])
        return items[0] if len(items) == 1 else ("seq", items)

    def item():
        kind, v = take()
        if kind == "word":
            weight = take()[1] if peek()[0] == "num" else 0.0
            e = ("word", v, weight)
        elif kind == "ref":
            e = ("ref", v)
        else:
            e = alt()
            close = take() if pos[0] < len(toks) else (None, None)
            if close != ("op", ")" if v == "(" else "]"):
                raise ValueError("grammar: '%s' is not closed" % v)
            if v == "[":
                e = ("opt", e)
        while peek() in (("op", "*"), ("op", "+")):
            e = ("star" if take()[1] == "*" else "plus", e)
        return e

    rules = {}
    while peek()[0] == "ref" and pos[0] + 1 < len(toks) and toks[pos[0] + 1] == ("op", "="):
        name = take()[1]
        take()
        if name in rules:
            raise ValueError("grammar: rule $%s is defined twice" % name)
        rules[name] = alt()
        if take() != ("op", ";") if pos[0] < len(toks) else True:
            raise ValueError("grammar: rule $%s does not end in ';'" % name)
    main = alt()
    if pos[0] != len(toks):
        raise ValueError("grammar: unexpected %r" % (toks[pos[0]][1],))
    return rules, main
