"""Regenerates INTEGRATION.md's appendix of environment switches from the sources (tests/test_abi.py checks that it is complete)."""
import re, glob, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
names = {}
live = set()   # read on a line that does not keep the answer in a `static`: every call (or every context) asks the environment again
for f in sorted(glob.glob(os.path.join(ROOT, 'morbit.jl_amd/csrc/*.hip')) + glob.glob(os.path.join(ROOT, 'morbit.jl_amd/csrc/*.hpp'))):
    for i, line in enumerate(open(f), 1):
        for m in re.finditer(r'mrbf_env\("(MRBF_[A-Z0-9_]+)"\)', line):
            names.setdefault(m.group(1), (os.path.basename(f), i))
            if not re.search(r'\bstatic\b', line.split("//")[0]):
                live.add(m.group(1))
rows = ["| `%s` | `csrc/%s:%d` |" % (n, names[n][0], names[n][1]) for n in sorted(names)]
head = "\n## Appendix: every environment switch the library reads"
txt = head + """

All of them are honoured only while `MRBF_EXPERIMENTS=1` is set (`mrbf_env()`, `csrc/common.hpp`); without it the library ignores its
whole `MRBF_*` environment. They exist for A/B runs, diagnostics and the tests that hold alternative implementations to the same
results; none is part of the interface. Where each one is read (the comment at that line says what it selects; regenerate this list
with `python tools/env_appendix.py`):

| switch | read at |
|---|---|
""" + "\n".join(rows) + """

When a change of the environment takes effect: `mrbf_env()` itself caches nothing, but most call sites keep the answer in a
`static const` and are frozen at their first use in the process. The following are asked again at every call -- or, for the
`MRBF_MEGA_*` schedule knobs and the values in `csrc/context.hip`, whenever a context is created -- so that a test can switch them
inside one process:

""" + ", ".join("`%s`" % n for n in sorted(live)) + ".\n"
p = os.path.join(ROOT, 'INTEGRATION.md')
s = open(p).read()
if head in s:
    s = s[:s.index(head)]
open(p, 'w').write(s.rstrip("\n") + "\n" + txt)
print(len(rows), "switches,", len(live), "read per call / per context")
