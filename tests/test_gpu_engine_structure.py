"""What the engine graph builder (csrc/engine.hip: rs_engine::build and its build_* sections, declared in csrc/engine_internal.h) builds under every structural switch,
precision and spec variant: ordered stage names, tensor count and the ordered tensor table (name | dtype | dims | halo) against
tests/golden/engine_structure.json.  The engine or trainer is created and inspected, no forward runs.  The configurations and the
fixture come from tools/parity/engine_manifest.py; on a deliberate change of the graph, rewrite the fixture with its --fixture."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("engine_manifest", os.path.join(ROOT, "tools", "parity", "engine_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load_tool()
CONFIGS = {c["name"]: c for c in M.configurations()}
with open(os.path.join(ROOT, "tests", "golden", "engine_structure.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_configuration():
    """No GPU needed: every configuration has an entry, the default's table is stored in full, and no recorded list is empty."""
    assert sorted(GOLDEN) == sorted(CONFIGS)
    assert "tensors" in GOLDEN[M.DEFAULT] and all("tensors_sha256" in g for n, g in GOLDEN.items() if n != M.DEFAULT and "error" not in g)
    for n, g in GOLDEN.items():
        if "error" not in g:
            assert g["stages"] and g["tensor_count"] > 0, n
            if CONFIGS[n]["kind"] == "trainer":
                assert g["trainer_stages"] and g["trainer_tensor_count"] > 0, n


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_engine_structure(gpu_required, name):
    env_before = dict(os.environ)
    rec = M.record(CONFIGS[name], structure_only=True)
    assert dict(os.environ) == env_before, "the configuration's switches were not restored"
    want = GOLDEN[name]
    if "error" in want or "error" in rec:
        assert rec.get("error") == want.get("error")
        return
    s = rec["structure"]

    def show(key):
        return f"{name}: {key} differs from tests/golden/engine_structure.json; now:\n" + "\n".join(s[key])

    assert s["net_shape"] == want["net_shape"]
    assert s["stages"] == want["stages"], show("stages")
    assert len(s["tensors"]) == want["tensor_count"], show("tensors")
    if "tensors" in want:
        assert s["tensors"] == want["tensors"], show("tensors")
    else:
        assert M.table_sha(s["tensors"]) == want["tensors_sha256"], show("tensors")
    if CONFIGS[name]["kind"] == "trainer":
        assert s["trainer_stages"], f"{name}: the trainer's own stage list is empty"
        assert s["trainer_stages"] == want["trainer_stages"], show("trainer_stages")
        assert len(s["trainer_tensors"]) == want["trainer_tensor_count"], show("trainer_tensors")
        assert M.table_sha(s["trainer_tensors"]) == want["trainer_tensors_sha256"], show("trainer_tensors")
