"""Register and scratch use of compiled kernels, without a GPU: hipcc cross-compiles a csrc file for
gfx950 with the kernel-resource-usage remarks, and the remarks are parsed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd")
HIPCC = "/opt/rocm/bin/hipcc"


def kernel_resources(source, tmp_path, extra_flags=()):
    """{mangled kernel name: {"VGPRs": n, "ScratchSize": bytes per lane, "Occupancy": waves per SIMD,
    "TotalSGPRs": n, ...}} of csrc/<source>, compiled as the Makefile compiles it plus extra_flags (the
    file's own flags there, if it has any)."""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *extra_flags,
                          "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-c",
                          os.path.join(PKG, "csrc", source), "-o", str(tmp_path / (source + ".o")),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)\b", line)  # units in brackets dropped
        if m and cur:
            res[cur][m.group(1)] = int(m.group(2))
    return res
