"""CPU tier: batched generation with images (aha_hip_generate_batch_mm) is wired through every layer -- public header, exported symbols
(as many as the header declares), ctypes table, Rust shim -- and its argument checks run before any device work."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generate_batch_mm_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_generate_batch_mm\(aha_model\* m, const uint32_t\* input_ids, const size_t\* seq_lens, size_t n_seqs,"
                     r"\s+const aha_mm_input\* const\* mm, const aha_sampling_params\* params, size_t max_new,"
                     r"\s+size_t max_tokens_per_pass, uint32_t\* tokens_out, size_t\* n_out, float\* step_logits_out\);", header)
    assert hasattr(hip_lib, "aha_hip_generate_batch_mm")
    assert len(_lib.SIGNATURES["aha_hip_generate_batch_mm"][1]) == 11
    # the header declares exactly what the library exports
    declared = set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(aha_hip_\w+)\(", header, re.M))
    nm = shutil.which("nm") or next((p for p in glob.glob("/opt/rocm*/llvm/bin/llvm-nm") + glob.glob("/opt/rocm*/lib/llvm/bin/llvm-nm")), None)
    assert nm, "no nm / llvm-nm on this machine"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("aha_hip_")}
    assert "aha_hip_generate_batch_mm" in declared and "aha_hip_generate_batch_mm" in exported
    assert len(declared) == len(exported) and declared == exported, (declared ^ exported)
    assert declared <= set(_lib.SIGNATURES)
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_generate_batch_mm\(\s*m: \*mut AhaModel,\s*ids: \*const u32,\s*seq_lens: \*const usize,"
                     r"\s*n_seqs: usize,\s*mm: \*const \*const AhaMmInput,\s*params: \*const AhaSamplingParams,\s*max_new: usize,"
                     r"\s*max_tokens_per_pass: usize,\s*tokens_out: \*mut u32,\s*n_out: \*mut usize,\s*step_logits_out: \*mut f32,?\s*\) -> i32;",
                     ext)
    assert re.search(r"pub fn generate_batch_mm\(\s*&mut self,\s*prompts: &\[&\[u32\]\],\s*mm: &\[MmInput<'_>\],"
                     r"\s*params: Option<&\[sys::AhaSamplingParams\]>,", src)


def test_generate_batch_mm_python_surface():
    import inspect

    from aha_amd import model
    sig = inspect.signature(model.HipInferenceModel.generate_batch_mm)
    assert list(sig.parameters) == ["self", "prompts", "data", "max_new", "params", "max_tokens_per_pass", "want_step_logits"]
    assert sig.parameters["params"].default is None and sig.parameters["max_tokens_per_pass"].default == 0
    assert callable(model.generate_generic_batch_mm)


def test_generate_batch_mm_null_arguments_fail_cleanly(hip_lib):
    """No GPU here: every call below is refused on its arguments alone."""
    from aha_amd import _lib
    from aha_amd.sampling import SamplingParams
    ids = (C.c_uint32 * 2)(1, 2)
    lens = (C.c_size_t * 1)(2)
    toks = (C.c_uint32 * 4)()
    n_out = (C.c_size_t * 1)()
    gen = hip_lib.aha_hip_generate_batch_mm
    assert gen(None, ids, lens, 1, None, None, 4, 0, toks, n_out, None) == -1
    assert b"null model" in hip_lib.aha_hip_last_error()
    assert gen(None, None, None, 0, None, None, 0, 0, None, None, None) == -1
    bad = SamplingParams(0.7).to_c()
    bad.repeat_penalty = 0.0
    arr = (_lib.SamplingParams * 1)(bad)
    assert gen(None, ids, lens, 1, None, arr, 4, 0, toks, n_out, None) == -1
    assert b"generate_batch_mm: params of sequence 0" in hip_lib.aha_hip_last_error()
    mm = (C.c_void_p * 1)()
    assert gen(None, ids, lens, 1, mm, None, 4, 0, toks, n_out, None) == -1
