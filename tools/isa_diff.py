"""Per-kernel comparison of two gfx950 device assemblies (hipcc <build flags> --cuda-device-only -S file.hip): has a refactor left the ISA alone?
usage: python tools/isa_diff.py <parent.s> <new.s> [--show N] [--rename REGEX=REPLACEMENT]...

Each file is split at its function labels (up to .Lfunc_end), comments and directives are dropped and the local labels (.LBB<n>_<m>, .Ltmp<n>, ...)
are renumbered in order of first appearance, so that a kernel that merely moved inside its translation unit compares equal. Per symbol of the parent:
  identical   the same instruction stream
  inverted    the same instruction count; line by line, every difference is a compare or a branch whose polarity flipped (s_cmp_eq <-> s_cmp_lg,
              s_cbranch_scc0 <-> scc1, vccz <-> vccnz, execz <-> execnz; the branch's target label may differ with it)
  DIFFERENT   anything else: the first N differing lines are shown (default 12)
  renamed    a symbol of the new file only whose mangled name differs from a parent-only symbol of the same base name just in its template arguments
              (a dropped argument that had one value left); the pair is then compared like any other
  gone / NEW  symbols of one file only
--rename REGEX=REPLACEMENT (repeatable, applied in order with re.sub to the PARENT's mangled names before anything is paired) says which symbol
of the new file a parent symbol became when the refactor changed its base name or added a template argument: two kernels merged under a flag,
say, which the `renamed` pairing cannot tell apart when several instantiations of one base name gain the same argument.
Exit status 1 when any symbol is DIFFERENT or NEW."""
import collections
import difflib
import re
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L(BB|tmp|JTI|func_begin|func_end)(\d+)(_\d+)?")
FLIP = [("s_cmp_eq_", "s_cmp_lg_"), ("s_cbranch_scc0", "s_cbranch_scc1"), ("s_cbranch_vccz", "s_cbranch_vccnz"), ("s_cbranch_execz", "s_cbranch_execnz")]


def functions(path):
    out, cur, buf, names = collections.OrderedDict(), None, [], {}
    for line in open(path):
        m = LABEL.match(line)
        if cur is None:
            if m and not line.startswith(".L"):
                cur, buf, names = m.group(1), [], {}
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = buf
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".L")):
            continue
        s = LOCAL.sub(lambda k: names.setdefault(k.group(0), ".L%d" % len(names)), s)
        buf.append(re.sub(r"\s+", " ", s))
    return out


def unflip(s):
    """polarity-free and label-free form of a compare / branch"""
    for a, b in FLIP:
        s = s.replace(b, a)
    return re.sub(r"\.L\d+", ".L", s)


def classify(a, b):
    if a == b:
        return "identical", []
    if len(a) == len(b):
        # line by line: every difference must be a compare or a branch whose polarity flipped (its target label may differ with it)
        changed = [(x, y) for x, y in zip(a, b) if x != y]
        if all(x.startswith(("s_cmp_", "s_cbranch_")) and unflip(x) == unflip(y) for x, y in changed):
            return "inverted", changed
    return "DIFFERENT", [x for x in difflib.unified_diff(a, b, lineterm="", n=0) if not x.startswith(("---", "+++"))]


def base(sym):
    """mangled name without its template arguments"""
    return re.split(r"I(?=L[ib]|N|\d)", sym, 1)[0]


def main(argv):
    show = int(argv[argv.index("--show") + 1]) if "--show" in argv else 12
    pa, pb = [x for x in argv[1:] if x.endswith(".s")][:2]
    a, b = functions(pa), functions(pb)
    renames = [argv[i + 1].split("=", 1) for i, x in enumerate(argv[:-1]) if x == "--rename"]
    was = collections.OrderedDict()       # name after the renames -> the parent's symbol
    for k in a:
        new = k
        for rx, to in renames:
            new = re.sub(rx, to, new)
        assert new not in was, f"--rename maps {was.get(new)} and {k} onto one name"
        was[new] = k
    a = collections.OrderedDict((new, a[k]) for new, k in was.items())
    bad = 0
    print(f"# {pa}: {len(a)} functions; {pb}: {len(b)} functions" + "".join(f" --rename '{rx}={to}'" for rx, to in renames))
    # a new-only symbol takes the place of the parent-only symbol of the same base name whose stream it matches best
    gone, renamed = [k for k in a if k not in b], {}
    for k in [k for k in b if k not in a]:
        rank = {"identical": 0, "inverted": 1, "DIFFERENT": 2}
        cands = sorted((rank[classify(a[g], b[k])[0]], g) for g in gone if base(g) == base(k) and g not in renamed.values())
        if cands:
            renamed[k] = cands[0][1]
    old_of = {v: k for k, v in renamed.items()}
    for k, fa in a.items():
        kb = k if k in b else old_of.get(k)
        if kb is None:
            print(f"gone       {k}")
            continue
        kind, delta = classify(fa, b[kb])
        note = f"  ({len(fa)} instructions" + (f", {len(delta)} compare / branch lines of opposite polarity)" if kind == "inverted" else ")")
        print(f"{kind:<10} {k}{note}" + (f"\n  --rename of {was[k]}" if was[k] != k else "") + (f"\n  renamed -> {kb}" if kb != k else ""))
        if kind == "DIFFERENT":
            bad += 1
            for x in delta[:show]:
                print("    " + x)
    for k in b:
        if k not in a and k not in renamed:
            print(f"NEW        {k}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
