"""The device check of k_wave.hip.h (tests/hip/wave_check.hip) is built with the library, lists its cases without a
device, and has a case for every instantiation of block_scan_array / block_scan_excl a kernel of the tree spells.
The run on the device is tests/test_gpu_wave_primitives.py."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clipper_amd", "csrc")


def expected_cases():
    """the case table: what wave_check --list must print, in its order"""
    names = [f"A.wave.{t}" for t in ("i32", "u32", "u64", "ull")]
    for waves in (4, 16):
        for t in ("u32", "i32", "u64"):
            names += [f"A.scan_excl<{waves}>.add.{t}", f"A.scan_excl<{waves}>.add.{t}.back_to_back"]
    for op in ("min", "max"):
        names += [f"A.scan_excl<4>.{op}.ull", f"A.scan_excl<4>.{op}.ull.back_to_back"]
    for threads, tag in ((256, "u64_u64.in_place"), (1024, "u32_u32.in_place"), (1024, "u32_u64"), (1024, "i32_i32"),
                         (1024, "i32_i32.out2")):
        for n in (0, 1, 63, 64, 65, threads - 1, threads, threads + 1, 2 * threads + 1, 3 * threads):
            names.append(f"A.scan_array<{threads}>.{tag}.n{n}")
    for rows in (1, 256):
        for n in (1, 1023, 1024, 1025, 2049):
            for out2 in ("no_out2", "out2"):
                for total in ("no_total", "total"):
                    if total == "total" and rows != 1:
                        continue
                    names.append(f"B.k_row_scan.rows{rows}.n{n}.{out2}.{total}")
    names += [f"B.k_slice_scan_small.n{n}" for n in (1, 1024, 1025, 32768)]
    names += [f"B.k_slice_scan_two_level.n{n}" for n in (32769, 262144, 262145, 2 * 262144 + 1025)]
    names += [f"B.k_slice_scan_both_paths.n{n}" for n in (32768, 32769)]
    names += [f"B.k_rv_scan.nb{n}" for n in (1, 1023, 1024, 1025, 2049)]
    names += [f"B.k_kg_slabs.dim{d}" for d in ("1x255x256", "257x1000x1", "256x257x1000", "1000x1x255", "255x256x257")]
    names += [f"B.k_kg_sum.n{n}" for n in (1, 255, 256, 257, 100000)]
    return names


def _built():
    from clipper_amd import build as b

    b.build_all()  # (up to date after build(): runs nothing then)
    return b.WAVE_CHECK


def _listed():
    out = subprocess.run([_built(), "--list"], capture_output=True, text=True, timeout=60,
                         env={k: v for k, v in os.environ.items() if k != "HIP_VISIBLE_DEVICES"} | {"HIP_VISIBLE_DEVICES": ""})
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.split("\n")[:-1]


def test_executable_is_built_and_git_ignored():
    exe = _built()
    assert os.path.isfile(exe) and os.access(exe, os.X_OK)
    rel = os.path.relpath(exe, ROOT)
    assert subprocess.run(["git", "-C", ROOT, "check-ignore", "-q", rel]).returncode in (0, 128), \
        f"{rel} is a built file and must be git-ignored"
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "tools/_bin/" in f.read().split()


def test_list_names_every_case_without_a_device():
    listed = _listed()
    assert len(set(listed)) == len(listed), "a case name appears twice"
    want = expected_cases()
    assert [n for n in want if n not in listed] == [], "cases of the table that --list does not name"
    assert [n for n in listed if n not in want] == [], "cases that the table does not hold"


def _constants(texts):
    """every `constexpr int NAME = <expression>;` of the sources, evaluated over the others"""
    raw = {}
    for text in texts.values():
        for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", text):
            raw[name] = expr

    def value(expr, depth=0):
        assert depth < 8, expr
        names = set(re.findall(r"[A-Za-z_]\w*", expr))
        if not re.fullmatch(r"[\w\s+\-*/()]+", expr) or not names <= set(raw):
            return None
        env = {n: value(raw[n], depth + 1) for n in names}
        if any(v is None for v in env.values()):
            return None
        return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, env))

    return value


def test_every_instantiation_at_a_call_site_has_a_case():
    texts = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hpp")) +
                       glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            texts[os.path.basename(path)] = re.sub(r"//[^\n]*", "", f.read())
    value = _constants(texts)
    listed = _listed()
    have = {fn: {int(n) for name in listed for n in re.findall(rf"A\.scan_{fn}<(\d+)>", name)} for fn in ("array", "excl")}
    sites = 0
    for fname, text in texts.items():
        for fn, arg in re.findall(r"\bblock_scan_(array|excl)\s*<([^<>]+)>", text):
            first = arg.split(",")[0].strip()
            if fname == "k_wave.hip.h" and fn == "excl" and first == "THREADS / 64":
                continue  # block_scan_array's own call, over its template parameter: covered through its cases
            n = value(first)
            assert n is not None, f"{fname}: block_scan_{fn}<{arg}>: cannot read the first template argument"
            assert n in have[fn], (f"{fname}: block_scan_{fn}<{arg}> (= {n}) has no case in tests/hip/wave_check.hip: "
                                   f"add one with this instantiation's types")
            sites += 1
    assert sites >= 8, "the call sites were not found: has the spelling changed?"
    assert have["array"] >= {256, 1024} and have["excl"] >= {4, 16}
