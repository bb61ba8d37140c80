"""The one rule the six host-frame entries size their batches by (siril-0.9_amd/csrc/sg_host_batch.hpp,
host only), pinned without a GPU at the batch sizes the entries had while each spelled the rule itself,
and the sources checked for the staging buffers and private helpers that the shared loop
(SgHostBatches, sg_ctx.hpp) retired.  tests/test_gpu_host_batches.py runs the loop past one batch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include "sg_host_batch.hpp"

int main(int argc, char **argv) {
	printf("%zu %zu\n", (size_t)SG_HOST_BUDGET_1G, (size_t)SG_HOST_BUDGET_512M);
	for (int i = 1; i + 3 < argc; i += 4)
		printf("%zu\n", sg_host_batch_frames(strtoull(argv[i], 0, 10), strtoull(argv[i + 1], 0, 10),
				strtoull(argv[i + 2], 0, 10), strtoull(argv[i + 3], 0, 10)));
	for (size_t v : {0, 1, 16, 17})
		printf("%zu\n", sg_up16(v));
	return 0;
}
'''

G1, M512 = 1 << 29, 1 << 28     # u16 elements: 1 GiB and 512 MiB
# (frames, elements per frame, budget, cap) -> frames per batch
CASES = [
    ((64, 4096 * 4096 * 1, G1, 0), 32),
    ((64, 4096 * 4096 * 1, M512, 0), 16),
    ((64, 4096 * 4096 * 3, G1, 0), 10),
    ((64, 32768 * 32768, G1, 0), 1),            # a frame above either budget still goes alone
    ((64, 32768 * 32768, M512, 0), 1),
    ((5, 40 * 48, G1, 0), 5),
    ((5, 40 * 48, G1, 2), 2),
    ((5, 40 * 48, G1, 7), 5),
    ((257, 9 * 67, G1, 128), 128),              # sg_prepro_frames: the cap is its device chunk
]


def test_the_batch_rule(tmp_path):
    src = tmp_path / "rule.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rule"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", SRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    args = [str(v) for case, _ in CASES for v in case]
    out = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0].split() == [str(G1), str(M512)]
    got = [int(v) for v in lines[1:1 + len(CASES)]]
    assert got == [want for _, want in CASES], list(zip(CASES, got))
    rest = [int(v) for v in lines[1 + len(CASES):] if v]
    assert rest == [0, 16, 16, 32]                              # sg_up16 of 0, 1, 16, 17


def _sources():
    for name in sorted(os.listdir(SRC)):
        with open(os.path.join(SRC, name)) as f:
            yield name, f.read()


def test_the_header_has_no_hip_in_it():
    text = dict(_sources())["sg_host_batch.hpp"]
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", text) == ["stddef.h"]
    assert not re.search(r"\bhip[A-Z_]", text)


def test_retired_names_are_gone():
    """one staging buffer (SgDevice::host_frames, which sg_prepro no longer has), one sg_up16, and the budgets
    spelled in sg_host_batch.hpp only"""
    for name, text in _sources():
        for old in ("fs_frames", "ecc_frames", "cosme_frames", "quality_frames", "pp->host_frames"):
            assert old not in text, (name, old)
        ups = re.findall(r"size_t (\w*up16)\(size_t", text)
        assert ups == (["sg_up16"] if name == "sg_host_batch.hpp" else []), (name, ups)
        if name in ("sg_findstar.hip", "sg_prepro.hip", "sg_ecc.hip", "sg_cosme.hip", "sg_quality.hip"):
            assert not re.search(r"1 << 2[89]", text), name
            assert "dv.host_frames" not in text, name            # the loop stages, not the entry
    ctx = dict(_sources())["sg_ctx.hpp"]
    assert len(re.findall(r"SgBuf host_frames;", ctx)) == 1


def test_retired_registration_variants_are_gone():
    """the registration variants that lost their A/B measurements went with the variables that selected them"""
    for name, text in _sources():
        for old in ("SG_REG_SPECP", "SG_REG_WCOLW", "SG_REG_XCD", "SG_REG_PB", "SG_REG_QAFTER", "SG_QGRAD_STREAM",
                    "SG_QGRAD_THREADS", "SG_REG_REFCONC", "SG_REG_COLOCC", "k_quality_grad("):
            assert old not in text, (name, old)
