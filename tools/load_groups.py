#!/usr/bin/env python3
"""Developer tool: the vector-memory loads of a kernel and the waits between them, from a `hipcc -S --cuda-device-only` listing.
For every basic block of a named kernel, in program order: each global/flat/buffer/scratch load (with its line in the listing), each
`s_waitcnt` that has a vmcnt(N), and how the block ends (branch or fall-through).  Loads with no wait and no block end between
them leave together; a vmcnt(0) between two loads is a dependent round trip.
Usage: load_groups.py file.s pattern...  (every kernel whose mangled name contains one of the patterns)"""
import re
import sys

LOAD = re.compile(r'^(global_load|flat_load|buffer_load|scratch_load)\w*')
WAIT = re.compile(r'^s_waitcnt\b.*vmcnt\((\d+)\)')
BRANCH = re.compile(r'^s_(cbranch\w*|branch|setpc_b64|endpgm)\b')


def blocks(body):
    """[(label, [(line_no, text)])] in program order"""
    out, cur, name = [], [], 'entry'
    for no, l in body:
        l = l.split(';')[0].strip()
        if not l or l[0] == '.' and not l.endswith(':'):
            continue
        if l.endswith(':'):
            out.append((name, cur))
            name, cur = l[:-1], []
            continue
        cur.append((no, l))
        if BRANCH.match(l) and not l.startswith('s_cbranch'):
            out.append((name, cur))
            name, cur = name + '+', []
    out.append((name, cur))
    return out


def report(name, body):
    print('== %s' % name)
    n_loads = n_waits = n_groups = 0
    for label, ins in blocks(body):
        rows, run = [], 0
        for no, l in ins:
            if LOAD.match(l):
                rows.append('  %6d  %s' % (no, ' '.join(l.split())))
                run += 1
                n_loads += 1
            elif WAIT.match(l):
                if run:
                    n_groups += 1
                rows.append('  %6d  -- wait vmcnt(%s)%s' % (no, WAIT.match(l).group(1), '   [after %d loads]' % run if run else ''))
                run = 0
                n_waits += 1
            elif l.startswith('s_cbranch'):
                if rows:
                    rows.append('  %6d  -- %s' % (no, ' '.join(l.split())))
        if any(r for r in rows if '-- s_cbranch' not in r):
            if run:
                n_groups += 1
            print(' %s:' % label)
            print('\n'.join(rows))
    print(' total: %d loads, %d vmcnt waits, %d load groups' % (n_loads, n_waits, n_groups))


def main():
    lines = open(sys.argv[1]).read().split('\n')
    pats = sys.argv[2:]
    i = 0
    while i < len(lines):
        m = re.match(r'^(_Z\w+):', lines[i])
        if m and (not pats or any(p in m.group(1) for p in pats)):
            j = i + 1
            while j < len(lines) and not lines[j].startswith('.Lfunc_end'):
                j += 1
            report(m.group(1), [(k + 1, lines[k]) for k in range(i + 1, j)])
            i = j
        i += 1


if __name__ == '__main__':
    main()
