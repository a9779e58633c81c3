#!/usr/bin/env python3
"""(kernel name, calls) tables of rocprofv3 --kernel-trace --stats runs of
tools/launch_probe.py, one per build, and whether they are equal.

  python3 tools/launch_table.py NAME=DIR [NAME=DIR ...] [--out FILE]

DIR: a rocprofv3 output directory (its newest *_kernel_stats.csv is read).
Prints one table with a calls column per build; exit status 1 if the columns
differ."""
import csv, glob, json, sys


def table(d):
    f = sorted(glob.glob(d + '/**/*_kernel_stats.csv', recursive=True))[-1]
    return {r['Name']: int(r['Calls']) for r in csv.DictReader(open(f))}


def main():
    args = [a for a in sys.argv[1:] if '=' in a]
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    tabs = {a.split('=', 1)[0]: table(a.split('=', 1)[1]) for a in args}
    names = sorted(set().union(*tabs.values()))
    same = all(t == next(iter(tabs.values())) for t in tabs.values())
    for n in names:
        print(' '.join('%6d' % t.get(n, 0) for t in tabs.values()), n)
    print('%d kernels, %s launches; tables %s' % (len(names), ' / '.join(str(sum(t.values())) for t in tabs.values()),
                                                  'equal' if same else 'DIFFER'))
    if out:
        with open(out, 'w') as f:
            json.dump({'equal': same, 'builds': list(tabs), 'calls': {n: [t.get(n, 0) for t in tabs.values()] for n in names}},
                      f, indent=0)
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
