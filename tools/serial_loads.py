"""Count the memory round trips a kernel makes before it starts computing.  A load the compiler left behind its own
`s_waitcnt vmcnt(0)` is one exposed trip to L2 / HBM; N independent loads that could have been issued together but
sit behind N such waits are N trips (tools/branchy_loads.py finds only the variant with a <= 4 instruction block behind
s_cbranch_execz).  Per kernel of a .hip file this prints the global / buffer loads and the DRAIN POINTS in front of the
first v_mfma (over the whole kernel if it has none): a drain point is an s_waitcnt containing vmcnt(0) that follows at
least one load not yet drained, counted in program order from the kernel entry - every path's blocks are counted, so
a kernel with two roles (k_x_moments' packing workgroups) shows the sum.  Only waits, loads and MFMAs are read.
    python tools/serial_loads.py [file.hip ...]"""
import os, re, subprocess, sys, tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dcase2019_task4_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
_LOAD = ("global_load", "buffer_load")


def compile_asm(path, out):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", path, "-o", out],
                   check=True, stderr=subprocess.DEVNULL)


def kernel_streams(asm_text):
    """{mangled kernel name: [instruction lines that are a wait, a load or an MFMA, in program order up to and including the first MFMA]}"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, re.M))
    out, kern, done = {}, None, False
    for line in asm_text.split("\n"):
        m = re.match(r"^(\w+):", line)
        if m and not line.startswith(".L"):
            kern, done = (m.group(1), False) if m.group(1) in kernels else (None, False)
            if kern:
                out[kern] = []
            continue
        if kern is None or done:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            kern = None
        elif t.startswith("v_mfma"):
            out[kern].append(t)
            done = True
        elif t.startswith("s_waitcnt") or t.startswith(_LOAD):
            out[kern].append(t)
    return out


def count(stream):
    """(loads, drain points) of one kernel's stream"""
    loads = drains = pending = 0
    for t in stream:
        if t.startswith(_LOAD):
            loads += 1
            pending += 1
        elif t.startswith("s_waitcnt") and "vmcnt(0)" in t and pending:
            drains += 1
            pending = 0
    return loads, drains


def demangle(names):
    res = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    short = []
    for d in res:
        d = d.split("(")[0]
        short.append(re.sub(r",\s+", ",", d[5:] if d.startswith("void ") else d))
    return dict(zip(names, short))


def analyze(files):
    """{kernel name as in the source, e.g. 'k_conv_wino<16,1>': (loads, drain points, stream)} over the given .hip files"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            path = f if os.path.isabs(f) or os.path.exists(f) else os.path.join(CSRC, f)
            out = os.path.join(tmp, os.path.basename(path) + ".s")
            compile_asm(path, out)
            streams = kernel_streams(open(out).read())
            if not streams:
                continue
            names = demangle(list(streams))
            for k, s in streams.items():
                res[names[k]] = count(s) + (s,)
    return res


if __name__ == "__main__":
    files = sys.argv[1:] or sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    for f in files:
        rows = analyze([f])
        for k, (loads, drains, s) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
            where = "first MFMA" if s and s[-1].startswith("v_mfma") else "end"
            print(f"{os.path.basename(f):12s} {drains:4d} drain points {loads:4d} loads before {where:10s}  {k}")
