"""profiles/topk_pfm_isa.txt: what hipcc made of reviews4rec_amd/csrc/topk_pfm.hip, per instantiation (compiled to gfx950
ISA here, no GPU needed), followed by tools/isa_scan.py's own lines for the unit:
  - registers (.amdhsa_next_free_vgpr, .amdhsa_accum_offset), scratch bytes and scratch instructions,
  - the dynamic LDS a launch asks for, from PfmTile's constants (head = the image of W, b, s, g, e; launch = head + the
    four waves' query rows where they live in LDS (KT >= 16) + the four waves' lists at K = 10 .. 128; no lists in the
    rank scan), and the occupancy that follows: waves per SIMD by registers (512 / VGPRs rounded up to 8), workgroups of
    four waves per CU by the 160 KiB of LDS at K = 10,
  - MFMA and instruction counts, and of the basic block of the per-slab loop that holds the MFMAs: its ds_read_b128, its
    s_waitcnt lgkmcnt(0), its v_readlane / v_writelane and its length,
  - per rank-scan instantiation from KT = 16 on: the loop block's s_waitcnt lgkmcnt(N) by N, and after how many of its
    MFMAs each lgkmcnt(0) stands.
`python tools/isa_table_pfm.py > profiles/topk_pfm_isa.txt`"""
import collections, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, 'reviews4rec_amd', 'csrc', 'topk_pfm.hip')
QT, WAVES, CU_LDS = 4, 4, 160 * 1024          # PFM_QT, PFM_WAVES of the unit; the LDS of a gfx950 CU

with tempfile.NamedTemporaryFile(suffix='.s') as tmp:
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', tmp.name, UNIT],
                   check=True, stderr=subprocess.DEVNULL)
    s = open(tmp.name).read()


def blocks_of(name):
    i = s.index(name + ':')
    out, cur = [], []
    for l in s[i:s.find('.Lfunc_end', i)].split('\n'):
        t = l.strip()
        if t.endswith(':') and t.startswith('.LBB'):
            out.append(cur)
            cur = []
        elif t and not t.startswith(('.', ';')):
            cur.append(t)
    return out + [cur]


count = lambda prefix, ins: sum(x.startswith(prefix) for x in ins)
print('# csrc/topk_pfm.hip compiled for gfx950 (hipcc -O3 -std=c++17 -S --cuda-device-only), by tools/isa_table_pfm.py (its\n'
      '# docstring has the columns).  QT = queries (pairs) per wave.  accum@ = where the AGPRs of the unified file begin.\n#')
print('# %-21s %3s %3s %2s | %5s %6s | %7s %3s | %6s %12s | %s | %5s %6s | %s'
      % ('kernel', 'KT', 'MT', 'QT', 'VGPRs', 'accum@', 'scratch', 'ops', 'head B', 'launch B', 'waves/SIMD, workgroups/CU by LDS',
         'MFMAs', 'instr', 'loop: b128 lgkmcnt(0) lane-ops / instr'))
total, waits = 0, []
for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', s, re.S):
    name, meta = m.group(1), m.group(2)
    blocks = blocks_of(name)
    ins = [x for b in blocks for x in b]
    vg = int(re.search(r'next_free_vgpr (\d+)', meta).group(1))
    ac = int(re.search(r'accum_offset (\d+)', meta).group(1))
    sc = int(re.search(r'private_segment_fixed_size (\d+)', meta).group(1))
    total += sc
    spills = sum('scratch_' in x for x in ins)
    k = re.search(r'(pfm_scan_kernel|rank_pfm_scan_kernel)ILi(\d+)ELi(\d+)E', name)
    if not k:
        short = re.sub(r'.*?(pair_kernel|rank_target_kernel|rank_excl_kernel).*', r'\1<PfmHead>', name)
        print('  %-27s -  - | %5d %6d | %7d %3d | %6d %12d | %32s | %5d %6d |' % (short, vg, ac, sc, spills, 0, 0, '', 0, len(ins)))
        continue
    kind, KT, MT = k.group(1), int(k.group(2)), int(k.group(3))
    KG = (KT + 3) // 4
    head = (KG * MT * 256 + 2 * MT * 16 + 2 * KG * 16) * 4                   # PfmTile::HEAD_FLOATS
    rows = WAVES * QT * KG * 16 * 4 if KT >= 16 else 0                       # PfmTile::Q_FLOATS per wave
    lists = lambda K: WAVES * QT * K * 8 if kind == 'pfm_scan_kernel' else 0
    launch = '%d' % (head + rows + lists(10)) + ('..%d' % (head + rows + lists(128)) if lists(10) else '')
    loop = max(blocks, key=lambda b: count('v_mfma', b))
    print('  %-21s %3d %3d %2d | %5d %6d | %7d %3d | %6d %12s | %14d %17d | %5d %6d | %4d %4d %4d / %d'
          % (kind, KT, MT, QT, vg, ac, sc, spills, head, launch, min(8, 512 // (-(-vg // 8) * 8)),
             CU_LDS // (head + rows + lists(10)), count('v_mfma', ins), len(ins), count('ds_read_b128', loop),
             sum('lgkmcnt(0)' in x for x in loop), count('v_readlane', loop) + count('v_writelane', loop), len(loop)))
    if kind == 'rank_pfm_scan_kernel' and KT >= 16:
        hist = collections.Counter(int(re.search(r'lgkmcnt\((\d+)\)', x).group(1)) for x in loop if 'lgkmcnt(' in x)
        done, at = 0, []
        for x in loop:
            done += x.startswith('v_mfma')
            if 'lgkmcnt(0)' in x:
                at.append(done)
        waits.append('# rank_pfm_scan_kernel<%d, %d>, s_waitcnt lgkmcnt(N) of the loop block by N: %s;\n'
                     '#   lgkmcnt(0) after %s of its %d MFMAs'
                     % (KT, MT, '  '.join('%d: %d' % kv for kv in sorted(hist.items())), ', '.join(map(str, at)), done))
print('# scratch bytes over all kernels: %d\n#' % total)
print('\n'.join(waits))
print('#\n# python tools/isa_scan.py topk_pfm.hip (kernels with scratch, >= 64 spilled scalars or >= 3 loads waited for at once;\n'
      '# spilled scalars live in vector lanes -- v_writelane / v_readlane, no memory):')
sys.stdout.flush()
subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_scan.py'), 'topk_pfm.hip'], check=True)
