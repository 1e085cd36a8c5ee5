"""Which kernels' machine code changed?  Compiles every csrc/*.hip to gfx950 assembly (hipcc -S, device only), hashes
each kernel's instruction stream (symbols, labels and comments normalised away, and without the section directive that
closes the kernel, so that a kernel may move into a header as a `static __global__`) and compares with a recorded baseline.
Baselines recorded before that directive was left out do not compare with hashes taken since.

    python tools/isa_guard.py --record profiles/r01_isa_hashes.json      # write the baseline
    python tools/isa_guard.py profiles/r01_isa_hashes.json               # list kernels that differ / are new

Used when an opt-in variant (a new template parameter) is added to a measured kernel: the default instantiation
must come out instruction for instruction as before, whatever its mangled name now is."""
import hashlib, importlib.util, json, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ddsp_amd', 'csrc')
# the flags the library ships with (ddsp_amd/build.py, loaded by path: the package itself needs torch and the built library)
_spec = importlib.util.spec_from_file_location('ddsp_amd_build', os.path.join(ROOT, 'ddsp_amd', 'build.py'))
build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build)
FLAGS = [f for f in build.FLAGS if f not in ('-shared', '-fPIC')] + ['-I' + os.path.join(ROOT, 'include'), '--cuda-device-only', '-S']


def demangled_kernels(asm_path):
  txt = open(asm_path).read()
  out = {}
  for m in re.finditer(r'^(_Z\w+):\s*; @\1\n(.*?)\n\.Lfunc_end\d+:', txt, re.S | re.M):
    body = re.sub(r'_Z\w+', 'SYM', m.group(2))
    body = re.sub(r'\.L\w+', 'LBL', body)
    lines = [line.split(';')[0].rstrip() for line in body.splitlines()]
    # the directive directly before .Lfunc_end says which section the assembler returns to behind the kernel: `.text`, or the
    # kernel's own section where it has internal linkage (a `static __global__` of a header).  It is no instruction.
    if lines and lines[-1].split()[:1] in (['.text'], ['.section']):
      lines.pop()
    body = '\n'.join(lines)
    out[m.group(1)] = hashlib.sha1(body.encode()).hexdigest()[:16]
  if not out:
    return out
  names = subprocess.run(['c++filt'] + list(out), capture_output=True, text=True).stdout.split('\n')
  return {re.sub(r'\(.*', '', n): h for n, h in zip(names, out.values())}


def current():
  hashes = {}
  names = sorted(n for n in os.listdir(CSRC) if n.endswith('.hip'))
  with tempfile.TemporaryDirectory() as tmp:
    def compile_one(name):
      asm = os.path.join(tmp, name + '.s')
      cmd = ['/opt/rocm/bin/hipcc'] + FLAGS + build.EXTRA_FLAGS.get(name, []) + [os.path.join(CSRC, name), '-o', asm]
      done = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
      if done.returncode:
        sys.exit('%s\n%s' % (' '.join(cmd), done.stderr))
      return demangled_kernels(asm)
    with ThreadPoolExecutor(max_workers=min(len(names), os.cpu_count() or 1)) as pool:
      for name, kernels in zip(names, pool.map(compile_one, names)):
        for kernel, h in kernels.items():
          hashes['%s: %s' % (name, kernel)] = h
  return hashes


if __name__ == '__main__':
  if len(sys.argv) == 3 and sys.argv[1] == '--record':
    json.dump(current(), open(sys.argv[2], 'w'), indent=1, sort_keys=True)
    print('recorded', sys.argv[2])
  else:
    base = json.load(open(sys.argv[1]))
    now = current()
    # a default instantiation keeps its hash when a defaulted template parameter is appended to its name
    base_hashes = set(base.values())
    changed = [k for k, h in now.items() if k in base and base[k] != h]
    new = [k for k, h in now.items() if k not in base and h not in base_hashes]
    renamed = [k for k, h in now.items() if k not in base and h in base_hashes]
    gone = [k for k, h in base.items() if k not in now and h not in set(now.values())]
    print('%d kernels, %d unchanged, %d renamed with identical code' % (len(now), len(now) - len(changed) - len(new) - len(renamed), len(renamed)))
    for title, items in (('CHANGED', changed), ('new', new), ('gone', gone)):
      for k in items:
        print('  %-8s %s' % (title, k))
    sys.exit(1 if changed or gone else 0)
