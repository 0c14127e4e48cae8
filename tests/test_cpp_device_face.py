"""The device face of include/lsdsort.hpp -- the wrappers over the device entries, which put a dozen positional arguments into
the C entries' slots in another order -- through tests/cpp/test_device_face.cpp: every wrapper called with every argument
observable, bit for bit against std::stable_sort references made in the program.  Its --no-device mode (the *_workspace_bytes
wrappers against the C functions, the argument checks made before a device is looked for) runs anywhere; the rest needs the GPU.
A guard keeps the face covered: every function the header defines in namespace lsd must be called by one of the C++ programs."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "lsdsort.hpp")
CPP_DIR = os.path.join(ROOT, "tests", "cpp")
HARNESSES = ("test_lsd_sort.cpp", "test_sharded.cpp", "test_device_face.cpp")


def _build_device_face(tmp_path):
    """The hipcc line of test_cpp_harness._build_sharded (host code only)."""
    exe = str(tmp_path / "test_device_face")
    libdir = os.path.join(ROOT, "lsdradixsort_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", INCLUDE, os.path.join(CPP_DIR, "test_device_face.cpp"),
                           "-o", exe, "-L", libdir, "-l:liblsdsort.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_device_face_without_a_device(tmp_path):
    """Builds everywhere; --no-device makes only calls that an argument check refuses (or with n = 0), so it touches no device
    even where there is one."""
    out = subprocess.run([_build_device_face(tmp_path), "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "device face test ok (--no-device)"


@pytest.mark.gpu
def test_device_face_on_the_device(tmp_path, gpu):
    """One run of the whole program: every wrapper, a created stream throughout, two virtual ranks, one hybrid-form shard."""
    out = subprocess.run([_build_device_face(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)                     # the program's own time per wrapper group
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "device face test ok"


def test_headers_stay_clean_as_c99_and_cxx11(tmp_path):
    """lsdsort.h is a C header (C99, -pedantic) and lsdsort.hpp asks for no more than C++11: both without a warning."""
    c_file, cxx_file = tmp_path / "face.c", tmp_path / "face.cpp"
    c_file.write_text('#include "lsdsort.h"\n')
    cxx_file.write_text('#include "lsdsort.hpp"\n')
    for cmd in (["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(c_file)],
                ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(cxx_file)]):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (" ".join(cmd), out.stderr[-3000:])


def _without_comments(source):
    source = re.sub(r"/\*.*?\*/", " ", source, flags=re.S)
    return re.sub(r"//[^\n]*", " ", source)


def _cut_namespace(source, name):
    """`source` without the bodies of `namespace <name> { ... }`."""
    while True:
        m = re.search(r"\bnamespace\s+" + name + r"\s*\{", source)
        if not m:
            return source
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(source[i], 0)
            i += 1
        source = source[:m.start()] + source[i:]


def defined_functions(header_text):
    """Names of the functions, member functions and constructors DEFINED (with a body) inside namespace lsd, `detail` left out:
    an identifier, its parameter list, at most `const` / `noexcept` / a constructor's initialisers, then the opening brace."""
    source = _cut_namespace(_without_comments(header_text), "detail")
    m = re.search(r"\bnamespace\s+lsd\s*\{", source)
    assert m, "namespace lsd"
    source = source[m.end():]
    names = set()
    for m in re.finditer(r"([~\w]+)\s*\(([^(){};]|\([^()]*\))*\)\s*(?:const\b\s*)?(?:noexcept\b\s*)?(?::[^{};]*)?\{", source):
        name = m.group(1)
        if name not in ("if", "for", "while", "switch", "catch", "static_assert", "sizeof") and not name.startswith("~"):
            names.add(name)
    return names


def called_in_harnesses(name, sources, classes):
    """A call of lsd::name(...), of a member (.name( / ->name( / communicator::name(), or, for a class, a mention of lsd::Class
    (which constructs it or catches it)."""
    if name in classes:
        return any(re.search(r"\blsd::" + name + r"\b", s) for s in sources)
    call = re.compile(r"(?:\blsd::|\bcommunicator::|\.|->)" + name + r"\s*(?:<[^;()]*>)?\s*\(")
    return any(call.search(s) for s in sources)


def _harness_sources():
    out = []
    for f in HARNESSES:
        with open(os.path.join(CPP_DIR, f)) as fh:
            out.append(_without_comments(fh.read()))
    return out


def uncovered(header_text):
    source = _without_comments(header_text)
    classes = set(re.findall(r"\b(?:class|struct)\s+(\w+)", source))
    sources = _harness_sources()
    return sorted(n for n in defined_functions(header_text) if not called_in_harnesses(n, sources, classes))


def test_every_wrapper_of_the_face_is_called_by_a_harness():
    with open(HEADER) as fh:
        header = fh.read()
    names = defined_functions(header)
    # the parser sees the face: were it to find nothing, the guard would pass for the wrong reason
    for known in ("sort", "sort_device", "sort_records_device", "topk", "topk16_device", "kth16_device", "sort_rows16_device",
                  "ran_hybrid_form", "loopback", "workspace_bytes", "rows16_workspace_bytes", "communicator", "status", "world"):
        assert known in names, (known, sorted(names))
    assert "key64_type" not in names, "namespace detail is left out"
    assert len(names) >= 30, sorted(names)
    assert uncovered(header) == [], "defined in namespace lsd and called by none of tests/cpp/*.cpp"
    # and it bites: a wrapper nobody calls is reported by name
    extra = header.replace("inline bool ran_hybrid_form(", "inline void sort_nothing_device(uint32_t* d_keys, size_t n) { (void)d_keys; (void)n; }\n"
                           "inline bool ran_hybrid_form(", 1)
    assert extra != header
    assert uncovered(extra) == ["sort_nothing_device"]
