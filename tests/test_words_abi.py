"""The visual-word exports without a device: null handles are refused, and the tree checks of msfm_voctree_create run in a
stand-alone program under the host sanitizers."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handles_are_refused():
    L = capi.lib()
    out = C.c_void_p()
    assert L.msfm_voctree_create(None, 10, 1, None, None, None, None, C.byref(out)) == A.MSFM_E_INVAL
    assert L.msfm_voctree_size(None, None, None, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_descset_words(None, None, 300, C.byref(out)) == A.MSFM_E_INVAL
    assert L.msfm_word_result_size(None, None, None, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_word_result_fetch(None, None, None, None, None, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_wordset_create_from_words(None, None, 0, C.byref(out)) == A.MSFM_E_INVAL
    L.msfm_voctree_destroy(None)
    L.msfm_word_result_destroy(None)
    assert not out.value


def test_tree_checks_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "words_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "words_host_check.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "words_host_check ok" in out.stdout
