"""Which kernel the output layer gets (csrc/out_plan.hpp: plan_out, plain C++) against the table of DESIGN section 1 and the
fall-backs of the paragraph under it, on the CPU: a stand-alone program built with g++ -fsanitize=address,undefined prints form,
kernel and grid for a list of facts; what must come out is written out here from the table, not computed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENERIC, F32, BK64, ROLLED, SMALL, PLANES, BF16X3, WHOLE = 1, 4096, 1024, 2048, 16384, 524288, 1048576, 16777216   # PAYNE_V_OUT_*


def facts(*parts, **kw):
    """The dicts `parts` and the keywords, later ones first."""
    out = {}
    for d in parts + (kw,):
        out.update(d)
    return out


FIELDS = ("variant", "n_cu", "b_max", "ld_hid", "w_out_kp", "n1", "n_layers", "n_out", "spectral", "freq", "sel", "dma_ok", "act_scale",
          "p3", "h2", "h2_freq", "pad", "pad_freq", "B")
# a 300-wide net (K = 320) with every operand set of its pixel rows built, on 256 compute units
BASE = facts(variant=0, n_cu=256, b_max=512, ld_hid=320, w_out_kp=320, n1=0, n_layers=3, n_out=4096, spectral=1, freq=0, sel=0, dma_ok=1,
             act_scale=1.0, p3=1, h2=1, h2_freq=0, pad=1, pad_freq=0, B=64)

MAIN = r'''
#include <cstdio>
#include "thepayne_amd/csrc/out_plan.hpp"
static const char* name(OutKernel k) {
  switch (k) {
    case OutKernel::GenericFused: return "payne_dense_kernel<64, 64, 32, true>";
    case OutKernel::Generic:      return "payne_dense_kernel<64, 64, 32, false>";
    case OutKernel::Dma32Nk10Ns4: return "payne_dense_dma_kernel<4, 32, 10, 4, true>";
    case OutKernel::Dma32Ns4:     return "payne_dense_dma_kernel<4, 32, 0, 4, true>";
    case OutKernel::Dma32Ns3:     return "payne_dense_dma_kernel<4, 32, 0, 3, false>";
    case OutKernel::Dma64Nk5:     return "payne_dense_dma_kernel<4, 64, 5, 3, true>";
    case OutKernel::Dma64:        return "payne_dense_dma_kernel<4, 64, 0, 3, true>";
    case OutKernel::Big3H2:       return "payne_dense_big3_kernel<true>";
    case OutKernel::Big3:         return "payne_dense_big3_kernel<false>";
    case OutKernel::Dma2hh5:      return "payne_dense_dma2hh_kernel<5>";
    case OutKernel::Dma2h5x64:    return "payne_dense_dma2h_kernel<5, 64>";
    case OutKernel::Dma2h10x32:   return "payne_dense_dma2h_kernel<10, 32>";
    case OutKernel::Dma2h0x32:    return "payne_dense_dma2h_kernel<0, 32>";
    case OutKernel::Dma3f10:      return "payne_dense_dma3f_kernel<10>";
    case OutKernel::Dma3Nk10Ns4:  return "payne_dense_dma3_kernel<10, 4, true>";
    case OutKernel::Dma3Ns4:      return "payne_dense_dma3_kernel<0, 4, true>";
    case OutKernel::Dma3Ns2:      return "payne_dense_dma3_kernel<0, 2, false>";
  }
  return "?";
}
int main() {
  static const char* forms[] = {"Generic", "F32Dma", "Bf16x3", "H2"};
  OutFacts f; int B, b[10];
  while (std::scanf("%u %d %d %d %d %d %d %d %d %d %d %d %f %d %d %d %d %d %d", &f.variant, &f.n_cu, &f.b_max, &f.ld_hid, &f.w_out_kp, &f.n1,
                    &f.n_layers, &f.n_out, &b[0], &b[1], &b[2], &b[3], &f.act_scale, &b[4], &b[5], &b[6], &b[7], &b[8], &B) == 19) {
    f.spectral = b[0]; f.freq = b[1]; f.sel = b[2]; f.dma_ok = b[3]; f.p3 = b[4]; f.h2 = b[5]; f.h2_freq = b[6]; f.pad = b[7]; f.pad_freq = b[8];
    const OutPlan o = plan_out(f, B);
    std::printf("%s|%s|%d|%d|%d\n", forms[(int)o.form], name(o.kernel), o.grid_m, o.grid_n, (int)o.sel);
  }
  return 0;
}'''

GEN_F, GEN = "payne_dense_kernel<64, 64, 32, true>", "payne_dense_kernel<64, 64, 32, false>"
DMA = "payne_dense_dma_kernel<4, %s>"
BIG_H2, BIG = "payne_dense_big3_kernel<true>", "payne_dense_big3_kernel<false>"
D2HH, D2H_64, D2H_10, D2H_0 = ("payne_dense_dma2hh_kernel<5>", "payne_dense_dma2h_kernel<5, 64>", "payne_dense_dma2h_kernel<10, 32>",
                               "payne_dense_dma2h_kernel<0, 32>")
D3F, D3_10, D3_0, D3_PLAIN = ("payne_dense_dma3f_kernel<10>", "payne_dense_dma3_kernel<10, 4, true>", "payne_dense_dma3_kernel<0, 4, true>",
                              "payne_dense_dma3_kernel<0, 2, false>")
K128 = facts(w_out_kp=128, ld_hid=128)                       # a 100-wide net
OWN = facts(B=64, n_out=4096)                                # 1 x 32 tiles of 64 x 128
MANY = facts(B=512, n_out=4224)                              # 8 x 33 = 264 tiles: more than 256 compute units
C5 = facts(B=512, n_out=32768)                               # 4 x 128 whole tiles of 128 x 256 = 2 a compute unit; 8 x 256 of 64 x 128
FREQ = facts(freq=1, h2_freq=1, pad_freq=1, n_out=1024, n1=1024)

# (what the case shows, facts that differ from BASE, form, kernel, grid_m, grid_n)
CASES = [
    # ---- DESIGN section 1, the table row by row
    ("hidden widths differ", facts(dma_ok=0), "Generic", GEN, 0, 0),
    ("two layers", facts(dma_ok=0, n_layers=2), "Generic", GEN_F, 0, 0),
    ("the continuum net", facts(spectral=0), "Generic", GEN, 0, 0),
    ("ld_hid < K", facts(ld_hid=288), "Generic", GEN, 0, 0),
    ("OUT_GENERIC", facts(variant=GENERIC), "Generic", GEN, 0, 0),
    ("OUT_F32, own CU, K = 320", facts(OWN, variant=F32), "F32Dma", DMA % "32, 10, 4, true", 1, 32),
    ("OUT_F32, own CU, OUT_ROLLED", facts(OWN, variant=F32 | ROLLED), "F32Dma", DMA % "32, 0, 4, true", 1, 32),
    ("OUT_F32, own CU, other K", facts(OWN, K128, variant=F32), "F32Dma", DMA % "32, 0, 4, true", 1, 32),
    ("OUT_F32, more tiles than CUs", facts(MANY, variant=F32), "F32Dma", DMA % "32, 0, 3, false", 8, 33),
    ("OUT_BK64, K = 320", facts(OWN, variant=BK64), "F32Dma", DMA % "64, 5, 3, true", 1, 32),
    ("OUT_BK64, K = 320, any batch", facts(MANY, variant=BK64 | F32), "F32Dma", DMA % "64, 5, 3, true", 8, 33),
    ("OUT_BK64, K = 320, OUT_ROLLED", facts(OWN, variant=BK64 | ROLLED), "F32Dma", DMA % "64, 0, 3, true", 1, 32),
    ("OUT_BK64, K = 128", facts(OWN, K128, variant=BK64), "F32Dma", DMA % "64, 0, 3, true", 1, 32),
    ("C5, H2", facts(C5), "H2", BIG_H2, 4, 128),
    ("C5, Bf16x3", facts(C5, variant=BF16X3), "Bf16x3", BIG, 4, 128),
    ("C5, OUT_PLANES", facts(C5, variant=PLANES), "Bf16x3", BIG, 4, 128),
    ("C5, OUT_SMALL_TILES", facts(C5, variant=SMALL), "H2", D2H_10, 8, 256),
    ("C5, a ragged batch", facts(C5, B=500), "H2", D2H_10, 8, 256),
    ("H2, K = 320, own CU", facts(OWN), "H2", D2HH, 1, 32),
    ("H2, K = 320, own CU, OUT_WHOLE_TILE", facts(OWN, variant=WHOLE), "H2", D2H_64, 1, 32),
    ("H2, K = 320, more tiles than CUs", facts(MANY), "H2", D2H_10, 8, 33),
    ("H2, K = 320, more tiles than CUs, OUT_WHOLE_TILE", facts(MANY, variant=WHOLE), "H2", D2H_10, 8, 33),
    ("H2, other K, own CU", facts(OWN, K128), "H2", D2H_0, 1, 32),
    ("H2, other K, more tiles than CUs", facts(MANY, K128), "H2", D2H_0, 8, 33),
    ("H2, K = 320, OUT_ROLLED", facts(OWN, variant=ROLLED), "H2", D2H_0, 1, 32),
    ("OUT_BF16X3, K = 320, own CU", facts(OWN, variant=BF16X3), "Bf16x3", D3F, 1, 32),
    ("OUT_PLANES, K = 320, own CU", facts(OWN, variant=PLANES), "Bf16x3", D3_10, 1, 32),
    ("OUT_BF16X3, other K, own CU", facts(OWN, K128, variant=BF16X3), "Bf16x3", D3_0, 1, 32),
    ("OUT_PLANES, other K, own CU", facts(OWN, K128, variant=PLANES), "Bf16x3", D3_0, 1, 32),
    ("OUT_BF16X3, K = 320, OUT_ROLLED, own CU", facts(OWN, variant=BF16X3 | ROLLED), "Bf16x3", D3_0, 1, 32),
    ("OUT_BF16X3, more tiles than CUs", facts(MANY, variant=BF16X3), "Bf16x3", D3_PLAIN, 8, 33),
    ("OUT_PLANES, more tiles than CUs", facts(MANY, variant=PLANES), "Bf16x3", D3_PLAIN, 8, 33),
    # ---- the paragraph under the table
    ("no calibration", facts(OWN, act_scale=0.0), "Bf16x3", D3F, 1, 32),
    ("no fp16 planes", facts(OWN, h2=0), "Bf16x3", D3F, 1, 32),
    ("activation plane of 2^31 bytes and more", facts(OWN, b_max=1 << 22), "Bf16x3", D3F, 1, 32),
    ("activation plane just below 2^31 bytes", facts(OWN, b_max=(1 << 22) - 1024, ld_hid=256, w_out_kp=256), "H2", D2H_0, 1, 32),
    ("weight plane of 2^31 bytes and more", facts(B=64, n_out=1 << 22, w_out_kp=256, ld_hid=256), "Bf16x3", D3_PLAIN, 1, 1 << 15),
    ("weight plane just below 2^31 bytes", facts(B=64, n_out=(1 << 22) - 1, w_out_kp=256, ld_hid=256), "H2", D2H_0, 1, 1 << 15),
    ("the resampled grid counts for the weight plane", facts(OWN, n1=1 << 22, w_out_kp=256, ld_hid=256), "Bf16x3", D3_0, 1, 32),
    ("no bf16 planes", facts(OWN, p3=0), "F32Dma", DMA % "32, 10, 4, true", 1, 32),
    ("no bf16 planes, OUT_BF16X3", facts(MANY, p3=0, variant=BF16X3), "F32Dma", DMA % "32, 0, 3, false", 8, 33),
    ("OUT_BK64, K % 64 != 0: as OUT_F32", facts(OWN, variant=BK64, w_out_kp=352, ld_hid=352), "F32Dma", DMA % "32, 0, 4, true", 1, 32),
    ("OUT_BK64, K % 64 != 0, more tiles than CUs", facts(MANY, variant=BK64, w_out_kp=352, ld_hid=352), "F32Dma", DMA % "32, 0, 3, false", 8, 33),
    ("rows of a resampled grid: no 128 x 256 tiles", facts(C5, FREQ, sel=1, n_out=30000, n1=32768), "H2", D2H_10, 8, 256),
    ("rows of a resampled grid, own CU: n1 columns", facts(FREQ, sel=1, B=24, n_out=700, n1=1024), "H2", D2HH, 1, 8),
    ("frequency rows", facts(FREQ, B=65), "H2", D2HH, 2, 8),
    ("frequency rows without their fp16 planes", facts(FREQ, B=65, h2_freq=0), "Bf16x3", D3F, 2, 8),
    ("frequency rows without their fp16 planes, OUT_PLANES", facts(FREQ, B=65, h2_freq=0, variant=PLANES), "Bf16x3", D3_10, 2, 8),
    ("OUT_ROLLED at K = 320, OUT_BK64", facts(MANY, variant=BK64 | ROLLED), "F32Dma", DMA % "64, 0, 3, true", 8, 33),
    ("own CU: exactly n_cu tiles", facts(B=64, n_out=256 * 128), "H2", D2HH, 1, 256),
    ("own CU: n_cu + 1 tiles", facts(B=64, n_out=256 * 128 + 1), "H2", D2H_10, 1, 257),
    ("own CU: exactly n_cu tiles, OUT_BF16X3", facts(B=128, n_out=128 * 128, variant=BF16X3), "Bf16x3", D3F, 2, 128),
    ("own CU: 3 x 86 tiles, OUT_BF16X3", facts(B=129, n_out=85 * 128 + 87, variant=BF16X3), "Bf16x3", D3_PLAIN, 3, 86),
    ("own CU: n_cu + 1 tiles, OUT_F32", facts(B=64, n_out=256 * 128 + 1, variant=F32), "F32Dma", DMA % "32, 0, 3, false", 1, 257),
    ("128 x 256 tiles: 2 n_cu - 1 of them", facts(B=128, n_out=511 * 256), "H2", D2H_10, 2, 1022),
    ("128 x 256 tiles: 2 n_cu of them", facts(B=128, n_out=512 * 256), "H2", BIG_H2, 1, 512),
    ("128 x 256 tiles: 2 n_cu of them on fewer compute units", facts(B=128, n_out=208 * 256, n_cu=104), "H2", BIG_H2, 1, 208),
]


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    d = tmp_path_factory.mktemp("out_plan")
    main, exe = d / "main.cpp", d / "out_plan_san"
    main.write_text(MAIN)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", ROOT,
                    str(main), "-o", str(exe)], check=True)
    lines = []
    for _, kw, *_ in CASES:
        assert set(kw) <= set(FIELDS), kw
        f = facts(BASE, **kw)
        if not f["n1"]:
            f["n1"] = f["n_out"]
        lines.append(" ".join(str(f[k]) for k in FIELDS))
    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(CASES), res.stdout
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_plan_is_the_table(planned, i):
    what, kw, form, kernel, grid_m, grid_n = CASES[i]
    assert planned[i] == "%s|%s|%d|%d|%d" % (form, kernel, grid_m, grid_n, kw.get("sel", 0)), (what, kw)


def test_the_table_names_every_kernel():
    """Every kernel of out_plan.hpp's OutKernel (one a comment line of the enumeration) is expected by some case above."""
    import re
    src = open(os.path.join(ROOT, "thepayne_amd", "csrc", "out_plan.hpp")).read()
    body = src[src.index("enum class OutKernel {"):]
    named = re.findall(r"^\s+\w+,?\s+// (payne_dense_\w+<[^>]*>)", body[:body.index("};")], re.M)
    assert len(named) == 17 and set(named) == {c[3] for c in CASES}
