"""Did a kernel behind an existing entry point move? Compares two device-assembly files of the library (gfx950), kernel by kernel:
every line of the function body and of its .amdhsa kernel descriptor, with the compiler's local label numbers and the kernel's own
symbol name normalised, so that a kernel whose mangled name gained a template argument still meets its former self.

    python -c "import __graft_entry__ as g; g.compile_hip('/tmp/parent.so', keep_asm='/tmp/parent.s')"    # in a checkout of the parent
    python -c "import __graft_entry__ as g; g.compile_hip('/tmp/this.so', keep_asm='/tmp/this.s')"        # in this tree
    python tools/compare_kernel_asm.py /tmp/parent.s /tmp/this.s [regex of the kernels to compare [regex of the new kernels]]

Prints one line per kernel (verdict, lines compared, sha256 prefix of either text, name) and the first lines of a difference; exits 1
if a kernel differs or is missing. The kernels to compare are those of the first file: by default the training kernels, "." for every
kernel and device function. A commit that adds kernels names them with the second regex: they are on one side only, listed and not
compared. The nothing_moved.txt files under profiles/ hold its output or its counts."""
import difflib
import hashlib
import re
import sys

TRAINING = (r"ppo_main_kernel|ppo_finish_kernel|ppo_finish_opt_kernel|ppo_finish_rows_kernel|ppo_adv|PpoGradK|PpoGradOptK|PpoGradRowsK|adam_update_kernel|"
            r"adam_norm_kernel|kl_control|mlp_backward_kernelINS_4MlpK|mlp_reduce|policy_act_kernel")


def functions(path):
    """({symbol: body lines}, {kernel: descriptor lines}) of an assembly file."""
    body, meta, cur, buf, kb = {}, {}, None, [], None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, buf = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                body[cur], cur = buf, None
                continue
            buf.append(line)
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            kb = meta[m.group(1)] = []
        elif line.strip().startswith(".amdhsa_") and kb is not None:
            kb.append(line.strip())
    return body, meta


def normalised(lines, name):
    out = []
    for l in lines:
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        l = re.sub(r"\.Ltmp\d+", ".Ltmp", l)
        l = re.sub(r"\.L__unnamed_\d+", ".L__unnamed", l)
        if l.strip().startswith((";", ".loc", ".file", ".cfi", ".text", ".section")):  # (a templated kernel sits in a comdat section)
            continue
        l = l.split(";")[0].rstrip().replace(name, "KERNEL")
        if l:
            out.append(l)
    return out


def key(name, new=None):
    """What a kernel is called on both sides; None for the kernels this comparison is not about (`new`: a regex of the new instantiations)."""
    if new and re.search(new, name):
        return None
    m = re.search(r"ppo_main_kernelILi(\d)ELb(\d)E", name)
    if m:
        return "ppo_main_kernel<%s, %s%s>" % (m.group(1), "float4" if m.group(2) == "1" else "generic", ", options" if "PpoOptMainK" in name else "")
    if "adam_update_kernel" in name:
        return "adam_update_kernel<gated>" if "AdamGatedK" in name else "adam_update_kernel"
    return name


def main():
    old_path, new_path = sys.argv[1], sys.argv[2]
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else TRAINING)
    new = sys.argv[4] if len(sys.argv) > 4 else None
    a, am = functions(old_path)
    b, bm = functions(new_path)
    A = {key(n, new): n for n in a if pat.search(n) and key(n, new)}
    B = {key(n, new): n for n in b if pat.search(n) and key(n, new)}
    same = 0
    for k in sorted(A):
        if k not in B:
            print("MISSING  ", k)
            continue
        x = normalised(a[A[k]], A[k]) + normalised(am.get(A[k], []), A[k])
        y = normalised(b[B[k]], B[k]) + normalised(bm.get(B[k], []), B[k])
        same += x == y
        digest = lambda t: hashlib.sha256("\n".join(t).encode()).hexdigest()[:16]  # noqa: E731
        print("identical" if x == y else "DIFFERS  ", "%5d lines" % len(x), digest(x), digest(y), k if k == A[k] == B[k] else "%s  [%s -> %s]" % (k, A[k], B[k]))
        if x != y:
            for d in list(difflib.unified_diff(x, y, lineterm="", n=0))[:20]:
                print("     ", d)
    print("%d of %d kernels are identical" % (same, len(A)))
    print("kernels only in the second file:")
    for n in sorted(set(b) - set(a)):
        if pat.search(n) and key(n, new) not in A:  # (the named new ones, and any other that has no former self)
            print("  ", n)
    return 0 if same == len(A) else 1


if __name__ == "__main__":
    sys.exit(main())
