# Dev tool: registers, scratch, LDS, instruction / MFMA counts and waves per SIMD of every kernel of csrc sources, from the device-only assembly.
#   bash tools/regs.sh patchconv [-DUDAPOSE_ELEM_F16]     one source of this tree
#   bash tools/regs.sh --ab [SOURCE...]                    parent (tools/_ab/oldtree, a git worktree of the parent commit) against this tree, both
#                                                          builds.  Every source is first compared as a whole file (apart from the __hip_cuid_ lines):
#                                                          "whole file identical"; only a file that differs gets one line per kernel "parent -> tree"
#                                                          with identical / differs.  Then the conditions (same kernel names, scratch stays 0, LDS and
#                                                          MFMA counts unchanged, no fewer waves per SIMD).  Default sources: the four convolution files
#                                                          and affine, fda, refine.  The parent's assembly is
#                                                          kept under /tmp/regs/parent and reused; remove that directory after moving the worktree.
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
asm() {     # asm TREE OUTDIR SOURCE FLAGS...: device-only assembly of one source
  local tree=$1 out=$2 f=$3; shift 3
  mkdir -p "$out" && (cd "$tree/uda_poseestimation_amd/csrc" && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value "$@" --cuda-device-only -S $f.hip -o "$out/$f.s" 2>&1 | grep -v -e "^$" -e "hip-link" | head -20)
}
if [ "$1" = "--ab" ]; then
  shift
  SRCS="${*:-igemm wgrad patchconv stem_dgrad affine fda refine}"
  for f in $SRCS; do
    for b in bf16 fp16; do
      D=; [ $b = fp16 ] && D=-DUDAPOSE_ELEM_F16
      ( [ -s /tmp/regs/parent/$b/$f.s ] || asm "$ROOT/tools/_ab/oldtree" /tmp/regs/parent/$b $f $D ) &
      asm "$ROOT" /tmp/regs/tree/$b $f $D &
    done
  done
  wait
  MODE=ab
else
  F=${1:-igemm}; shift
  asm "$ROOT" /tmp/regs/one $F "$@"
  MODE=one; SRCS=$F
fi
python3 - $MODE $SRCS <<'PY'
import re, sys

def kernels(path):
    """name -> (fields, instruction texts) of every kernel of one assembly file"""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, re.S):
        name, desc = m.group(1), m.group(2)
        d = lambda k: int(re.search(r'\.amdhsa_%s (\d+)' % k, desc).group(1))
        body = txt[txt.index('\n%s:' % name):m.start()]                                 # (the descriptor follows the kernel's code)
        ins = [l.split(';')[0].strip() for l in body.split('\n')]
        ins = [l for l in ins if l and not l.startswith('.') and not l.endswith(':')]
        c = lambda k: int(re.search(r'; %s: (\d+)' % k, txt[m.end():]).group(1))       # the compiler's summary comment behind the descriptor
        out[name] = ({'vgpr': d('next_free_vgpr'), 'accoff': d('accum_offset'), 'sgpr': c('TotalNumSgprs'),
                      'scratch': d('private_segment_fixed_size'), 'lds': d('group_segment_fixed_size'), 'ins': len(ins),
                      'mfma': sum(1 for l in ins if l.startswith('v_mfma')), 'waves': c('Occupancy')}, ins)
    return out

KEYS = ('vgpr', 'accoff', 'sgpr', 'scratch', 'lds', 'ins', 'mfma', 'waves')
short = lambda n: n[:150]
if sys.argv[1] == 'one':
    for n, (f, _) in kernels('/tmp/regs/one/%s.s' % sys.argv[2]).items():
        print(short(n), ' '.join('%s %d' % (k, f[k]) for k in KEYS))
    sys.exit(0)
bad = 0
for src in sys.argv[2:]:
    for b in ('bf16', 'fp16'):
        old, new = kernels('/tmp/regs/parent/%s/%s.s' % (b, src)), kernels('/tmp/regs/tree/%s/%s.s' % (b, src))
        strip = lambda p: [l for l in open(p) if '__hip_cuid_' not in l]      # whole file, apart from the per-file __hip_cuid_ symbol lines
        if strip('/tmp/regs/parent/%s/%s.s' % (b, src)) == strip('/tmp/regs/tree/%s/%s.s' % (b, src)):
            print('## %s %s: whole file identical' % (src, b))
            continue
        print('## %s %s: %d kernels; names %s' % (src, b, len(new), 'equal' if set(old) == set(new) else 'DIFFER'))
        bad += set(old) != set(new)
        for n in new:
            if n not in old:
                continue
            (fo, io), (fn, i_n) = old[n], new[n]
            mn = lambda ins: [l.split()[0] for l in ins]
            verdict = 'identical' if io == i_n else ('differs (registers only)' if mn(io) == mn(i_n) else 'differs')
            broke = [k for k, t in (('scratch', fo['scratch'] == 0 and fn['scratch'] != 0), ('lds', fo['lds'] != fn['lds']), ('mfma', fo['mfma'] != fn['mfma']),
                                    ('waves', fn['waves'] < fo['waves'])) if t]
            bad += len(broke)
            print(short(n), ' '.join('%s %s' % (k, fo[k] if fo[k] == fn[k] else '%d->%d' % (fo[k], fn[k])) for k in KEYS), verdict,
                  ('CONDITION BROKEN: ' + ','.join(broke)) if broke else '')
print('conditions: %s' % ('all hold' if not bad else '%d BROKEN' % bad))
PY
