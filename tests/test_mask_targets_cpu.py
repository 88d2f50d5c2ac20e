"""The mask-target switch without a GPU: the command line's default, the trainers' argument check, the C header's declarations, and the
closed form's edge rule (csrc/mask_targets.h) compiled for the host against the host rasteriser of librs_engine.so."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from proj_roadsurf_amd.engine import LIB_PATH, MultiScaleTrainer, Trainer, load_library
from proj_roadsurf_amd.spec import EngineSpec
from tests.mask_target_cases import FAMILIES, family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_default_is_host():
    from proj_roadsurf_amd.train_model import build_parser
    assert build_parser().parse_args(["config.yaml"]).mask_targets == "host"
    assert build_parser().parse_args(["config.yaml", "--mask-targets", "device"]).mask_targets == "device"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["config.yaml", "--mask-targets", "gpu"])


@pytest.mark.parametrize("value", ["gpu", "Device", "", None])
def test_trainers_reject_other_values(value):
    """Checked before the library is loaded or a device is touched."""
    spec = EngineSpec(num_classes=2)
    with pytest.raises(ValueError, match="mask_targets"):
        Trainer(spec, {}, (128, 128, 3), mask_targets=value)
    with pytest.raises(ValueError, match="mask_targets"):
        MultiScaleTrainer(spec, {}, (128, 128, 3), [192], mask_targets=value)


def test_header_declares_the_three_functions():
    hdr = open(os.path.join(ROOT, "include", "rs_engine.h")).read()
    for name in ("rs_trainer_set_polygons", "rs_trainer_mask_backward_device", "rs_op_mask_targets"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+RS_POLYGONS_DO_NOT_FIT\s+1\b", hdr) and re.search(r"#define\s+RS_ABI_VERSION\s+1\b", hdr)


HOST_DRIVER = r"""
#include "mask_targets.h"
#include <cstddef>
#include <vector>
extern "C" void mt_host_entries(const double* polys, const long long* poly_off, const int* poly_len, const int* inst_first,
                                const int* entry_inst, const float* boxes, int n_entries, int S, unsigned char* out) {
  std::vector<int> cnt(S * S + S + 1);
  for (int e = 0; e < n_entries; ++e) {
    unsigned char* o = out + (size_t)e * S * S;
    const MtBox b = mt_box(boxes[4 * e], boxes[4 * e + 1], boxes[4 * e + 2], boxes[4 * e + 3], S);
    const int g = entry_inst[e];
    for (int q = inst_first[g]; q < inst_first[g + 1]; ++q) {
      const double* p = polys + poly_off[q];
      const int k = poly_len[q] / 2;
      cnt.assign(cnt.size(), 0);
      for (int j = 0; j < k; ++j)
        for (int m = 0; m < S; ++m) {
          const int j2 = j + 1 == k ? 0 : j + 1;
          int xs, ys, xe, ye;
          mt_vertex(b, p[2 * j], p[2 * j + 1], &xs, &ys);
          mt_vertex(b, p[2 * j2], p[2 * j2 + 1], &xe, &ye);
          const int pt = mt_edge_point(xs, ys, xe, ye, m, S);
          if (pt >= 0) ++cnt[pt];
        }
      int par = 0;
      for (int c = 0; c < S * S; ++c) { par ^= cnt[c] & 1; if (par) o[(c % S) * S + c / S] = 1; }
    }
  }
}
"""


@pytest.fixture(scope="module")
def host_closed_form(tmp_path_factory):
    """csrc/mask_targets.h (the functions the kernel calls per (edge, column) pair) compiled for the host, no mul+add contraction."""
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    d = tmp_path_factory.mktemp("mt_host")
    (d / "driver.cpp").write_text(HOST_DRIVER)
    so = str(d / "libmt_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "proj_roadsurf_amd", "csrc"),
                    str(d / "driver.cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.mark.parametrize("name", FAMILIES)
def test_closed_form_equals_the_host_rasteriser(host_closed_form, name):
    """The rules of the kernel, run on the CPU, give the masks of rs_rasterize_entries on every family of the GPU test."""
    from proj_roadsurf_amd.train_targets import rasterize_entries
    load_library()
    n = 32 if name == "far" else 128
    instances, ent, boxes = family(name, n, seed=1)
    want = rasterize_entries(instances, ent, boxes, 28)
    arrs = [np.asarray(p, np.float64).reshape(-1) for polys in instances for p in polys]
    lens = np.array([a.size for a in arrs], np.int32)
    off = np.zeros(len(arrs), np.int64)
    off[1:] = np.cumsum(lens[:-1])
    flat = np.ascontiguousarray(np.concatenate(arrs))
    first = np.zeros(len(instances) + 1, np.int32)
    first[1:] = np.cumsum([len(p) for p in instances])
    ent = np.ascontiguousarray(ent, np.int32)
    boxes = np.ascontiguousarray(boxes, np.float32)
    out = np.zeros((n, 28, 28), np.uint8)
    host_closed_form.mt_host_entries.restype = None
    host_closed_form.mt_host_entries.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    host_closed_form.mt_host_entries(flat.ctypes.data, off.ctypes.data, lens.ctypes.data, first.ctypes.data, ent.ctypes.data, boxes.ctypes.data, n, 28,
                                     out.ctypes.data)
    assert np.array_equal(out.astype(bool), want) and want.any()
