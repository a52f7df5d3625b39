"""The search kernels keep their resources under the PUCT rule options: agz_engine.hip is
cross-compiled for gfx950 with the Makefile's flags (the device half only) and the compiler's resource report must show no scratch for the
kernels that descend trees or write pi rows (none has any today) and no occupancy below the
parent's.  CPU only; skipped where there is no hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphago.jl_amd", "csrc")
# kernel -> the occupancy [waves/SIMD] it has had since DESIGN.md section 5k (analysis and review search in k_pre / k_post)
KERNELS = {"k_pre": 2, "k_post": 5, "k_tree_op": 2, "k_tree_pruned_pi": 8, "k_tree_gumbel_pi": 8}


def _hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cand = re.search(r"^HIPCC \?= (\S+)", mk, flags=re.M).group(1)
    return os.environ.get("HIPCC") or (cand if os.path.exists(cand) else shutil.which("hipcc"))


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*)$", mk, flags=re.M).group(1).replace("$(EXTRA)", "").split()
    rule = re.search(r"agz_engine\.o:.*\n\t\$\(HIPCC\) \$\(FLAGS\) (.*?) -c ", mk).group(1).split()
    return flags + rule


def test_search_kernels_have_no_scratch_and_keep_their_occupancy(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    flags = _flags()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, "agz_engine.hip"),
                                          "-o", str(tmp_path / "agz_engine.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = block.split()[0]
        m = re.match(r"_ZN3agz\d+(k_[a-z_]+?)E", name)
        if not m or m.group(1) not in KERNELS:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        seen[m.group(1)] = dict(vgprs=get("VGPRs"), sgprs=get("SGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                                occupancy=get("Occupancy [waves/SIMD]"))
    print(seen)
    assert set(seen) == set(KERNELS), sorted(set(KERNELS) - set(seen))
    for k, v in seen.items():
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= KERNELS[k], (k, v)
