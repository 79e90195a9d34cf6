"""Per (kernel name, grid, workgroup): the launch counts of two rocprofv3 --kernel-trace csv directories, and where they differ."""
import collections, csv, glob, json, sys
def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(f) == 1, f
    rows = list(csv.DictReader(open(f[0])))
    c = collections.Counter()
    for r in rows:
        g = tuple(int(r[k]) for k in r if k.lower().startswith("grid_size"))
        w = tuple(int(r[k]) for k in r if k.lower().startswith("workgroup_size"))
        c[(r["Kernel_Name"], g, w)] += 1
    return c, len(rows)
a, na = load(sys.argv[1]); b, nb = load(sys.argv[2])
diff = {str(k): (a.get(k, 0), b.get(k, 0)) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}
names = collections.Counter(); [names.update({k[0].split("(")[0][:60]: v}) for k, v in b.items()]
print("TRACECMP " + json.dumps({"parent_kernels": na, "new_kernels": nb, "distinct_name_grid_workgroup": len(set(a) | set(b)),
                                "equal": not diff, "differences": diff, "new_by_name": dict(names)}))
