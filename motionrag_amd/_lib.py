"""ctypes binding of libmrag_hip.so (the C ABI declared in include/mrag_hip.h).

The library is the product: there is NO CPU fallback anywhere in this package.  `lib()` raises
`HipLibraryMissing` when the shared object has not been built, and every op in `ops.py` raises when
handed a non-GPU tensor.  Build with `python -m motionrag_amd._lib` (or `__graft_entry__.build()`):
hipcc cross-compiles for gfx950 without a GPU present.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_HERE, "libmrag_hip.so")
# compiled in this order, at most MAX_COMPILERS at a time: the long units first, so that none of them starts late behind the short ones
SOURCES = ["gemm_tiled.hip", "gemm_w4.hip", "topk_scan.hip", "gemm_conv.hip", "attn16.hip", "topk_dense.hip", "topk_mfma.hip", "attn_flash.hip", "attn_varlen.hip", "gemm_skinny.hip", "gemm_fp8.hip", "gemm_mxfp6.hip", "ff_fused.hip", "conv_fp8.hip", "api.hip", "gemm_bf16.hip", "gemm_k320.hip", "attn_fp8.hip",
           "comm.hip", "norm.hip", "pointwise.hip", "preprocess.hip", "unet_ops.hip", "cama_seq.hip", "attn_ip_folded.hip", "attn_bf16.hip", "attn_hd.hip", "attn_small.hip", "attn_tiny.hip", "topk.hip", "probe.hip"]
MAX_COMPILERS = 16
ABI_VERSION = 11
# per-file flags: the SLP vectoriser packs the softmax row-sum adds into v_pk_add_f32 + shuffles (slower beside MFMAs)
EXTRA_FLAGS = {f: ["-fno-slp-vectorize"] for f in ("attn_flash.hip", "attn_varlen.hip", "attn_tiny.hip", "attn_ip_folded.hip", "attn_bf16.hip", "attn16.hip", "attn_fp8.hip", "attn_hd.hip")}


class HipLibraryMissing(RuntimeError):
    pass


# The C ABI is written down once, in include/mrag_hip.h; this table is the only hand-written part of its Python side.
_SCALARS = {"int": c_int32, "int32_t": c_int32, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t"}      # what a pointer that travels as c_void_p may point at
_DECLARATOR = re.compile(r"(\**)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?")


def _ctype(const, base, stars, structs, decl):
    """the ctypes type of `[const] base` behind `stars` asterisks; anything outside the table raises, naming the declaration"""
    if not stars and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and const and base == "char":
        return c_char_p
    if stars == 1 and const and base in structs:
        return POINTER(structs[base])
    if stars == 2 and base == "void":
        return POINTER(c_void_p)
    if stars == 1 and base in _POINTEES:
        return c_void_p
    raise ValueError(f"mrag_hip.h: no ctypes mapping for the type of `{decl}`")


def _fields(body, structs):
    """`const void *A, *W; int64_t M, N, K; float scale[4];` -> [(name, ctype)]: the asterisks and the array bound belong to each declarator"""
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(const\s+)?(\w+)\b\s*(.*)", decl, re.S)
        parts = [_DECLARATOR.fullmatch(p.strip()) for p in m.group(3).split(",")] if m else [None]
        if not all(parts):
            raise ValueError(f"mrag_hip.h: cannot read the declaration `{decl}`")
        for d in parts:
            t = _ctype(m.group(1), m.group(2), len(d.group(1)), structs, decl)
            out.append((d.group(2), t * int(d.group(3)) if d.group(3) else t))
    return out


def _value(expr, decl):
    """an integer literal, a parenthesised negative one, or `a << b`; no eval"""
    m = re.fullmatch(r"(\d+)|\(\s*(-\d+)\s*\)|(\d+)\s*<<\s*(\d+)", expr.strip())
    if not m:
        raise ValueError(f"mrag_hip.h: cannot read the value of `{decl}`")
    return int(m.group(3)) << int(m.group(4)) if m.group(3) else int(m.group(1) or m.group(2))


def parse_header(text: str):
    """The ABI a header's TEXT declares, as three tables in header order:
         structs    {C name: ctypes.Structure subclass}  from every `typedef struct NAME { ... } NAME;` (a later struct may point at an earlier one)
         prototypes {name: (restype, [argtypes])}        from every `RET mrag_name(args);`
         constants  {name: int}                          from every `#define MRAG_X <int>` and every enumerator
       A type, a value expression or a `mrag_*(` declaration it cannot read raises ValueError: a guessed width would shift a kernel's argument block."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    structs, prototypes, constants = {}, {}, {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        structs[m.group(3)] = type(m.group(3), (Structure,), {"_fields_": _fields(m.group(2), structs)})
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(MRAG_\w+)[ \t]+(\S.*)$", text, re.M):
        constants[m.group(1)] = _value(m.group(2), m.group(0).strip())
    for m in re.finditer(r"\benum\b\s*\w*\s*\{(.*?)\}", text, re.S):
        nxt = 0
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            name, _, expr = (p.strip() for p in item.partition("="))
            if not re.fullmatch(r"\w+", name):
                raise ValueError(f"mrag_hip.h: cannot read the enumerator `{item}`")
            constants[name] = nxt = _value(expr, item) if expr else nxt
            nxt += 1
    for m in re.finditer(r"(?<![\w*])(const\s+)?(\w+)\s*(\**)\s*\b(mrag_\w+)\s*\(([^()]*)\)\s*;", text):
        decl = " ".join(m.group(0).split())
        args = []
        for part in (p.strip() for p in m.group(5).split(",")):
            a = re.fullmatch(r"(const\s+)?(\w+)\b\s*(\**)\s*\b(\w+)", part)
            if a:
                args.append(_ctype(a.group(1), a.group(2), len(a.group(3)), structs, decl))
            elif part != "void" or args:
                raise ValueError(f"mrag_hip.h: cannot read the parameter `{part}` of `{decl}`")
        prototypes[m.group(4)] = (_ctype(m.group(1), m.group(2), len(m.group(3)), structs, decl), args)
    for name in re.findall(r"\b(mrag_\w+)\s*\(", text):
        if name not in prototypes:
            raise ValueError(f"mrag_hip.h: `{name}(` is declared in a form the binding cannot read")
    return structs, prototypes, constants


with open(os.path.join(_HERE, "..", "include", "mrag_hip.h")) as _fh:          # read once, at import (source_hash() needs it at load anyway)
    STRUCTS, PROTOTYPES, CONSTANTS = parse_header(_fh.read())
SYMBOLS = list(PROTOTYPES)            # every entry point the header declares (tests check the .so exports exactly these)
MRAG_OK, MRAG_EINVAL, MRAG_ENOTSUP = (CONSTANTS[n] for n in ("MRAG_OK", "MRAG_EINVAL", "MRAG_ENOTSUP"))

# the argument blocks under the names the package uses
GemmArgs, GemmFp8Args, FfFusedArgs = STRUCTS["mrag_gemm_args"], STRUCTS["mrag_gemm_fp8_args"], STRUCTS["mrag_ff_fused_args"]
AttnArgs, AttnVarlenArgs, LnArgs = STRUCTS["mrag_attn_args"], STRUCTS["mrag_attn_varlen_args"], STRUCTS["mrag_ln_args"]
QkNormRopeArgs, GroupNormArgs = STRUCTS["mrag_qknorm_rope_args"], STRUCTS["mrag_groupnorm_args"]
ConvArgs, ConvFp8Args, ResizePatchArgs = STRUCTS["mrag_conv_args"], STRUCTS["mrag_conv_fp8_args"], STRUCTS["mrag_resize_patch_args"]
ResamplerLayer, ResamplerArgs = STRUCTS["mrag_resampler_layer"], STRUCTS["mrag_resampler_args"]
EncoderLayer, CamaEncoderArgs = STRUCTS["mrag_encoder_layer"], STRUCTS["mrag_cama_encoder_args"]

_lib = None


def source_hash() -> str:
    """digest of what the library is built from: every file of csrc/, include/mrag_hip.h and the per-file compile flags (sha256, 16 hex digits).
    The build stamps it into the binary (`mrag_source_hash()`); `lib()` refuses a binary whose stamp differs -- modification times are not
    consulted (a checkout, a copy to the GPU box or a variant build can leave a stale binary NEWER than the sources)."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(_CSRC) if f.endswith((".hip", ".h")))
    for f in files:
        h.update(f.encode() + b"\0")
        with open(os.path.join(_CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.join(_HERE, "..", "include", "mrag_hip.h"), "rb") as fh:
        h.update(b"mrag_hip.h\0" + fh.read())
    h.update(repr((SOURCES, sorted(EXTRA_FLAGS.items()), os.environ.get("MRAG_EXTRA_HIPCC_FLAGS", ""))).encode())
    return h.hexdigest()[:16]


def binary_stamp(path: str) -> str:
    """the source digest a built library carries, read from the file's bytes (no dlopen); '' when absent"""
    try:
        with open(path, "rb") as fh:
            blob = fh.read()
    except OSError:
        return ""
    i = blob.find(b"MRAG_SOURCE_HASH=")
    if i < 0:
        return ""
    j = blob.find(b"\0", i)
    return blob[i + 17:j].decode("ascii", "replace")


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into motionrag_amd/libmrag_hip.so (in-tree; needs no GPU).  Rebuilds whenever the binary's stamp is not
    the digest of the sources beside it.  MRAG_EXTRA_HIPCC_FLAGS (extra hipcc flags, e.g. -DMRAG_DIAG_VMCNT0; see tools/README.md) is part of the digest."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    want = source_hash()
    if os.path.exists(LIB_PATH) and binary_stamp(LIB_PATH) == want:
        return LIB_PATH
    extra = os.environ.get("MRAG_EXTRA_HIPCC_FLAGS", "").split()
    build_dir = os.path.join(_HERE, "build")
    os.makedirs(build_dir, exist_ok=True)
    import hashlib
    hdr = hashlib.sha256()
    for f in sorted(f for f in os.listdir(_CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "mrag_hip.h")]:
        with open(os.path.join(_CSRC, f), "rb") as fh:
            hdr.update(fh.read())
    jobs = []
    for src in SOURCES:
        obj = os.path.join(build_dir, src.replace(".hip", ".o"))
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment"] + EXTRA_FLAGS.get(src, []) + extra + (
            [f'-DMRAG_SOURCE_HASH="{want}"'] if src == "api.hip" else []) + ["-c", os.path.join(_CSRC, src), "-o", obj]
        objs.append(obj)
        # incremental: an object is reused when its source, the shared headers and its command line are what they were when it was compiled
        with open(os.path.join(_CSRC, src), "rb") as fh:
            key = hashlib.sha256(fh.read() + hdr.digest() + " ".join(cmd).encode()).hexdigest()
        tag = obj + ".key"
        if os.path.exists(obj) and os.path.exists(tag) and open(tag).read() == key:
            continue
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        if os.path.exists(tag):
            os.remove(tag)
        jobs.append((src, cmd, tag, key))

    def compile_one(job):
        src, cmd, tag, key = job
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if res.returncode != 0:
            return f"hipcc failed on {src}:\n{res.stdout.decode()}"
        with open(tag, "w") as fh:
            fh.write(key)

    with ThreadPoolExecutor(max_workers=MAX_COMPILERS) as pool:       # (started in SOURCES order)
        failed = [err for err in pool.map(compile_one, jobs) if err]
    if failed:
        raise RuntimeError("\n".join(failed))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs + ["-ldl"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if res.returncode != 0:
        raise RuntimeError(f"link failed:\n{res.stdout.decode()}")
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load the C-ABI library; fail loudly when it is missing or stale (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -m motionrag_amd._lib` (hipcc, gfx950). "
            "motionrag_amd has no CPU fallback.")
    # torch ships its own libamdhip64.so: it must be the HIP runtime of the process (it owns the streams and the
    # device memory handed to the kernels), so make sure it is loaded BEFORE our library resolves the same soname.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    L.mrag_abi_version.restype = c_int32
    L.mrag_target_arch.restype = c_char_p
    if L.mrag_abi_version() != ABI_VERSION:
        raise HipLibraryMissing(f"{LIB_PATH} has ABI {L.mrag_abi_version()}, expected {ABI_VERSION}: rebuild")
    L.mrag_source_hash.restype = c_char_p
    have = L.mrag_source_hash().decode()
    try:
        want = source_hash()
    except OSError as e:                                                     # a binary-only install: nothing to compare the stamp with
        raise HipLibraryMissing(f"{LIB_PATH} carries stamp {have} but the sources it must be checked against are not readable ({e})") from e
    if have != want:
        raise HipLibraryMissing(f"{LIB_PATH} was built from other sources (stamp {have}, sources beside it {want}): rebuild with "
                                "`python -m motionrag_amd._lib` -- a stale or variant binary is never loaded silently")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


class HipError(RuntimeError):
    pass


def check(rc: int, what: str) -> None:
    if rc != 0:
        kind = {MRAG_EINVAL: "MRAG_EINVAL", MRAG_ENOTSUP: "MRAG_ENOTSUP"}.get(rc, f"hipError {rc}")
        raise HipError(f"{what} failed: {kind}")


if __name__ == "__main__":
    print(build(verbose=True))
