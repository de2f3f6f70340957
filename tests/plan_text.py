"""mpx_describe_plan's text, shared by test_plan_cpu.py, test_gpu_plan.py and golden/make_plan_digests.py: the two-call read, the records
of a section, and the per-section counts and digests that tests/golden/plan_digests.json holds."""
import ctypes as C
import hashlib

# every section mpx_describe_plan prints, in its order (include/mpx.h); a line's first word is its section
SECTIONS = ("engine", "conv", "ops", "ops_bt", "ops_pt", "ops_pt0", "tail", "ptail", "norm", "dw", "lnorm", "attn", "se", "shuffle", "pool3c")


def describe(lib, arch_id):
    """(rc, text) of mpx_describe_plan(arch_id) by the two-call idiom; text is None when rc != 0."""
    n = C.c_size_t(0)
    rc = lib.mpx_describe_plan(arch_id, None, 0, C.byref(n))
    if rc:
        return rc, None
    buf = C.create_string_buffer(n.value + 1)
    rc = lib.mpx_describe_plan(arch_id, buf, n.value + 1, C.byref(n))
    return rc, (buf.value.decode() if rc == 0 else None)


def by_section(text):
    """{section: [line, ...]} in the text's order; every section of SECTIONS is a key."""
    out = {s: [] for s in SECTIONS}
    for line in text.splitlines():
        out[line.split(" ", 1)[0]].append(line)     # KeyError: a section this module does not know
    return out


def records(lines):
    """The key=value pairs of a section's lines as dicts of strings."""
    return [dict(kv.split("=", 1) for kv in line.split(" ") if "=" in kv) for line in lines]


def digests(text):
    """{section: {"n": records, "sha256": digest of its lines}} -- what the golden file holds per architecture."""
    return {s: {"n": len(lines), "sha256": hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest()}
            for s, lines in by_section(text).items()}
