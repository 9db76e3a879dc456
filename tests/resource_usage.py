"""Register, LDS and scratch figures of the kernels of one source file, as the compiler reports them (shared by the
resource-usage gates of the CPU tests; a plain module like ewald_ref.py)."""
import copy
import functools
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resource_usage(source):
    """{kernel name: {field: value}} from hipcc -Rpass-analysis=kernel-resource-usage with the library's own flags, for
    the file `source` of torch_nfft_amd/csrc, which must be one of the library's sources.  Compiled once per file and
    test run; every caller gets a copy of its own."""
    return copy.deepcopy(_resource_usage(source))


@functools.lru_cache(maxsize=None)
def _resource_usage(source):
    spec = importlib.util.spec_from_file_location("_nfft_hip_build", os.path.join(ROOT, "torch_nfft_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert source in build.SOURCES
    cmd = [build.HIPCC] + build.FLAGS + ["--cuda-device-only", "-x", "hip", "-c", os.path.join(build.CSRC, source),
                                         "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    usage, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return usage
