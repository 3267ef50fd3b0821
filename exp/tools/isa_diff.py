#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel: the proof a refactor of het_amd/csrc owes.

    git worktree add /tmp/parent HEAD~1
    python3 exp/tools/isa_diff.py /tmp/parent/het_amd/csrc het_amd/csrc [--rename 8CsrItems=5Items] [--rename-re 'REGEX=REPL']
                                  [--keep DIR] [-j N]

Compiles every file of the Makefile's SRCS in both trees with the Makefile's flags plus --cuda-device-only -S and compares
the set of kernel symbols and the text of every kernel, label to .end_amdhsa_kernel (descriptor included).  --rename
rewrites a substring of the OLD tree's assembly first (a renamed parameter type changes the mangled names).  The
--rename-re maps the OLD tree's kernels by their DEMANGLED names (c++filt), for a change that plain substitution on mangled names
cannot follow -- a template argument added to a kernel turns parameter types into substitutions (PKT_) and renumbers the ones
after them: e.g. --rename-re '(HET_rgat_\w+_fwd)_bf16<=\1<unsigned short, ' --rename-re '(HET_rgat_\w+_fwd)<(?!unsigned)=\1<float, '.  With
it both trees' kernels are keyed by demangled name and the symbol in the kernel's own text (its .amdhsa_kernel line) is replaced by
that key; everything else is compared as it is.  The per-translation-unit __hip_cuid_<hash> symbol lies outside the kernels and is not compared.  One summary line per file;
exit status 1 when anything differs.

--local-labels: block labels are .LBB<n>_<block> with n the function's ordinal in its module, so a kernel ADDED to a file renumbers
the labels of every kernel emitted after it (and, where the number gains a digit, the padding in front of the label's comment).
With this flag the ordinal and that padding are dropped before the comparison; instructions, operands, block numbers and the
kernel descriptors are compared as they are."""
import argparse
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import isa_stats  # noqa: E402


LOCAL_LABELS = False


def kernels(path):  # isa_stats' parser also returns device functions and data labels: keep what ends in a kernel descriptor
    ks = {k: b for k, b in isa_stats.kernels(path).items() if b and b[-1].strip().startswith(".end_amdhsa_kernel")}
    if LOCAL_LABELS:
        ks = {k: [re.sub(r"\s+;", " ;", re.sub(r"BB\d+_", "BB_", line)) for line in b] for k, b in ks.items()}
    return ks


def by_demangled(ks, renames):  # {symbol: body} -> {demangled (and renamed) name: body with the symbol replaced by it}, names changed
    names = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True, check=True).stdout.split("\n")
    out, changed = {}, 0
    for (sym, body), name in zip(ks.items(), names):
        key = name
        for pat, to in renames:
            key = re.sub(pat, to, key)
        changed += key != name
        assert key not in out, key
        out[key] = [line.replace(sym, key) for line in body]
    return out, changed


def make_var(csrc, name):
    m = re.search(rf"^{name}\s*\??:?=\s*(.*)$", (Path(csrc) / "Makefile").read_text(), re.M)
    return m.group(1).strip()


def assemble(csrc, src, out):
    flags = make_var(csrc, "CXXFLAGS").replace("$(ARCH)", make_var(csrc, "ARCH")).replace("$(GIT_SHA)", "isa_diff").replace('\\"', '"')
    out.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([make_var(csrc, "HIPCC"), *flags.split(), "--cuda-device-only", "-S", src, "-o", str(out)], cwd=csrc, check=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--rename-re", action="append", default=[], metavar="REGEX=REPL", help="on the old tree's demangled kernel names")
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--local-labels", action="store_true", help="ignore the function ordinal in block labels (see above)")
    a = ap.parse_args()
    global LOCAL_LABELS
    LOCAL_LABELS = a.local_labels
    tmp = Path(a.keep or tempfile.mkdtemp(prefix="isa_diff_"))
    srcs = make_var(a.new, "SRCS").split()
    if srcs != make_var(a.old, "SRCS").split():
        print("SRCS differ between the trees")
        return 1
    with ThreadPoolExecutor(a.j) as ex:
        jobs = [(s, ex.submit(assemble, a.old, s, tmp / "old" / (s + ".s")), ex.submit(assemble, a.new, s, tmp / "new" / (s + ".s"))) for s in srcs]
        files = [(s, o.result(), n.result()) for s, o, n in jobs]
    bad = 0
    for s, o, n in files:
        text = o.read_text()
        renamed = 0
        for r in a.rename:
            frm, to = r.split("=")
            renamed += len({k for k in kernels(o) if frm in k})
            text = text.replace(frm, to)
        o.write_text(text)
        ko, kn = kernels(o), kernels(n)
        if a.rename_re:
            ko, changed = by_demangled(ko, [r.split("=", 1) for r in a.rename_re])
            kn, renamed = by_demangled(kn, [])[0], renamed + changed
        only_old, only_new = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
        differ = sorted(k for k in set(ko) & set(kn) if ko[k] != kn[k])
        same = len(set(ko) & set(kn)) - len(differ)
        print(f"{s}: {len(ko)} kernels compared, {same} identical, {renamed} renamed, {len(differ)} differ, {len(only_old)} only old, {len(only_new)} only new")
        for tag, names in (("differs", differ), ("only old", only_old), ("only new", only_new)):
            for k in names:
                print(f"    {tag}: {k}")
        bad += len(differ) + len(only_old) + len(only_new)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
