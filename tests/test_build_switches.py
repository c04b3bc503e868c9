"""The shipped kernels carry no developer build switches.

A tuning session's scaffolding (ablation bits, cycle stamps, A/B alternatives, dispatcher overrides spelt -DMI_…) is
folded to its verdict before it is committed: the only MI_ macros a preprocessor conditional under csrc/ may name are the
headers' include guards and the two that arrange gemm_f32.hip's translation units.  Source text only.
"""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "matrix-multiplication_amd" / "csrc"
CONDITIONAL = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")
ARRANGE_UNITS = {"MI_GEMM_TU_NAME", "MI_GEMM_SINGLE_TU"}  # which kernels a unit holds, never a second code path


def test_no_conditional_names_a_build_switch():
    files = sorted(p for p in CSRC.iterdir() if p.is_file())
    assert len(files) > 40, "csrc/ not found where the package keeps it"
    offending = []
    for path in files:
        for no, line in enumerate(path.read_text().splitlines(), 1):
            m = CONDITIONAL.match(line)
            if not m:
                continue
            names = re.findall(r"\bMI_\w+", m.group(1).split("//")[0])
            if any(not (n.endswith("_H_") or n in ARRANGE_UNITS) for n in names):
                offending.append(f"{path.name}:{no}: {line.strip()}")
    assert not offending, "build switches in shipped sources:\n" + "\n".join(offending)
