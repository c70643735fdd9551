"""Register / scratch / LDS / occupancy table of every kernel of libgq as the COMPILER allocates them (rocprofv3's kernel-trace
`vgpr` column reports the allocation granule, not the allocation).

    python tools/kernel_resources.py [out.md] [--keep-asm /tmp/gq_kernels.s] [--parts JOBS]
    python tools/kernel_resources.py [out.md] --lib libgq.so [--against other/libgq.so]

Compiles csrc/gq_kernels.hip for gfx950 with the product's flags plus -Rpass-analysis=kernel-resource-usage (device side only), parses
the remarks and counts the scratch_load / scratch_store instructions of each kernel in the assembly.  As ONE translation unit holding every
variant (the default: a quarter of an hour since the flat self-collision scene comes in three builds) - or, with --parts JOBS, as the
product library is built: one unit per part of csrc/Makefile (-DGQ_PART=k), JOBS of them side by side, a few minutes; the allocator sees
what it sees in the product, and the table is the library's.

--lib reads a BUILT library instead (no GPU, no compile): the gfx950 code objects out of its .hip_fatbin, their metadata notes (VGPRs, SGPRs,
scratch bytes per lane, spills, LDS) and the kernels' symbol sizes (code bytes); --against lists the kernels that differ from another
library's, or are in one of the two only - how a change shows that it left the existing kernels alone."""
import collections, concurrent.futures, re, struct, subprocess, sys, tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / 'gym_quadruped_amd' / 'csrc'


def product_flags():
    """the Makefile's device flags (include paths relative to CSRC)"""
    return subprocess.run(['make', '-s', '-C', str(CSRC), 'print-flags'], check=True, capture_output=True, text=True).stdout.split()


def short(name):
    d = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
    d = re.sub(r'^void ', '', d)
    d = re.sub(r'\(.*\)$', '', d)
    return d.replace('gq::', '')


LLVM = Path('/opt/rocm/llvm/bin')
LIB_COLS = ('VGPRs', 'SGPRs', 'scratch B/lane', 'SGPR spills', 'VGPR spills', 'LDS B', 'code bytes')


def lib_table(lib):
    """kernel (demangled, short) -> the LIB_COLS values, from the gfx950 code objects bundled in `lib`"""
    rows = {}
    with tempfile.TemporaryDirectory() as td:
        fat = Path(td) / 'fatbin'
        subprocess.run([str(LLVM / 'llvm-objcopy'), f'--dump-section=.hip_fatbin={fat}', str(lib)], check=True)
        d = fat.read_bytes()
        for k, m in enumerate(re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', d)):
            at = m.start() + 32
            for _ in range(struct.unpack_from('<Q', d, m.start() + 24)[0]):
                off, size, tl = struct.unpack_from('<QQQ', d, at)
                triple = d[at + 24:at + 24 + tl]
                at += 24 + tl
                if not (triple.startswith(b'hip') and b'gfx950' in triple and size):
                    continue
                co = Path(td) / f'co{k}'
                co.write_bytes(d[m.start() + off:m.start() + off + size])
                sizes = {}
                for line in subprocess.run(['nm', '-S', str(co)], check=True, capture_output=True, text=True).stdout.splitlines():
                    f = line.split()
                    if len(f) == 4 and f[2] in 'Tt':
                        sizes[f[3]] = int(f[1], 16)
                notes = subprocess.run([str(LLVM / 'llvm-readobj'), '--elf-output-style=GNU', '--notes', str(co)], check=True, capture_output=True, text=True).stdout
                for blk in re.split(r'\n\s*- \.agpr_count', notes)[1:]:
                    g = lambda key: re.search(rf'\.{key}:\s+(\S+)', blk).group(1)
                    name = g('name').strip("'")
                    rows[short(name)] = (int(g('vgpr_count')), int(g('sgpr_count')), int(g('private_segment_fixed_size')), int(g('sgpr_spill_count')),
                                         int(g('vgpr_spill_count')), int(g('group_segment_fixed_size')), sizes.get(name, -1))
    return rows


def lib_main(out_md, lib, against):
    mine = lib_table(lib)
    head = '| kernel | ' + ' | '.join(LIB_COLS) + ' |\n|' + '---|' * (len(LIB_COLS) + 1)
    row = lambda k, v: f'| `{k}` | ' + ' | '.join(str(x) for x in v) + ' |'
    text = f'# Kernel resources of {Path(lib).name} (gfx950 code objects: metadata notes and symbol sizes)\n\n'
    if against:
        other = lib_table(against)
        same = sorted(k for k in mine if other.get(k) == mine[k])
        text += (f'{len(other)} kernels in the other library, {len(mine)} in this one; {len(same)} are identical in every column.\n\n'
                 '## Kernels that differ\n\n' + head.replace('| kernel |', '| kernel | library |').replace('|---|', '|---|---|', 1) + '\n')
        for k in sorted(set(mine) | set(other)):
            if other.get(k) != mine.get(k):
                for tag, t in (('other', other), ('this', mine)):
                    if k in t:
                        text += row(k, t[k]).replace(f'`{k}` |', f'`{k}` | {tag} |') + '\n'
        text += '\n## Every kernel of this library\n\n'
    text += head + '\n' + '\n'.join(row(k, mine[k]) for k in sorted(mine)) + '\n'
    if out_md:
        out_md.write_text(text)
    print(text)


def main(argv):
    out_md = Path(argv[0]) if argv and not argv[0].startswith('--') else None
    if '--lib' in argv:
        return lib_main(out_md, argv[argv.index('--lib') + 1], argv[argv.index('--against') + 1] if '--against' in argv else None)
    keep = Path(argv[argv.index('--keep-asm') + 1]).resolve() if '--keep-asm' in argv else None
    jobs = int(argv[argv.index('--parts') + 1]) if '--parts' in argv else 0
    nparts = int(re.search(r'^NPARTS = (\d+)', (CSRC / 'Makefile').read_text(), re.M).group(1))
    units = [[f'-DGQ_PART={k}', f'-DGQ_NPARTS={nparts}'] for k in range(nparts)] if jobs else [[]]
    with tempfile.TemporaryDirectory() as td:
        def compile_unit(k):
            asm = Path(td) / f'k{k}.s'
            r = subprocess.run(['/opt/rocm/bin/hipcc', *product_flags(), *units[k], '-gline-tables-only', '-Rpass-analysis=kernel-resource-usage', '-S',
                                '--cuda-device-only', '-o', str(asm), 'gq_kernels.hip'], capture_output=True, text=True, cwd=CSRC)
            if r.returncode:
                sys.exit(r.stderr[-3000:])
            return r.stderr, asm.read_text()
        with concurrent.futures.ThreadPoolExecutor(max(jobs, 1)) as pool:
            done = list(pool.map(compile_unit, range(len(units))))
        if keep:
            keep.write_text(''.join(a for _, a in done))
        rows, cur = collections.OrderedDict(), None
        for line in ''.join(e for e, _ in done).splitlines():
            m = re.search(r'remark: Function Name: (\S+)', line)
            if m:
                cur = m.group(1); rows[cur] = {}
                continue
            m = re.search(r'remark:\s+([A-Za-z][\w ]*?)(?: \[[\w/]+\])?: (\d+)', line)
            if m and cur:
                rows[cur][m.group(1).strip()] = int(m.group(2))
        scratch, fn = collections.Counter(), None
        for line in ''.join(a for _, a in done).splitlines():
            m = re.match(r'^(_Z\w+):', line)
            if m:
                fn = m.group(1)
            elif fn and re.match(r'\s*scratch_(load|store)', line):
                scratch[fn] += 1
    lines = ['| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | scratch instr. (static) | LDS B | occupancy (waves/SIMD) |', '|---|---|---|---|---|---|---|---|']
    for fn, d in rows.items():
        lines.append(f"| `{short(fn)}` | {d.get('VGPRs', '?')} | {d.get('AGPRs', '?')} | {d.get('TotalSGPRs', '?')} | {d.get('ScratchSize', '?')} | {scratch.get(fn, 0)} | "
                     f"{d.get('LDS Size', '?')} | {d.get('Occupancy', '?')} |")
    text = ('# Kernel resources as allocated by the compiler (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, product flags; '
            + (f'the {nparts} build parts of csrc/Makefile, as in the product library' if jobs else 'ONE translation unit holding every variant') + ')\n\n'
            'step_kernel<SOLVER, MODE, CONE, BOXES, SELF, PRIM, PERSIST>: SOLVER 1 Newton / 0 PGS; MODE 0 production, 1 instrumented, 2 stage cut.\n'
            'mailbox_step_kernel<SOLVER, CONE, BOXES, SELF, PRIM>: the closed-loop persistent rollout.\n'
            'step_kernel_prim<SOLVER, MODE, CONE, PERSIST> / mailbox_step_kernel_prim<SOLVER, CONE>: the flat self-collision scene without the convex block '
            '(SCENE_FLAT_SELF_PRIM); the one without the box routines (SCENE_FLAT_SELF_HULL) is step_kernel<.., BOXES false, SELF true, PRIM false, ..>.\n\n' + '\n'.join(lines) + '\n')
    if out_md:
        out_md.write_text(text)
    print(text)


if __name__ == '__main__':
    main(sys.argv[1:])
