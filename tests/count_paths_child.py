"""Child process of tests/test_count_paths_gpu.py: counts the files of a manifest with the library LSQ_LIB names -- the
developer build, whose LSQ_ABLATE and LSQ_GRID_WGS switches are read at every count -- and writes tables and path counters
as JSON.  usage: python count_paths_child.py manifest.json out.json

manifest: {"options": {name: value}, "files": [{"name", "interval", "map", "mrf", "R", "grids": [null | n, ...], "modes": [256, 288]}]}
out:      {name: {"<grid>/<mode>": {"cnt", "bases", "dbg", "exceptions", "recounted", "reads_per_look", "compact", "pool"}}}"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lesseq_amd as L      # noqa: E402


def main(manifest, out_path):
    with open(manifest) as f:
        man = json.load(f)
    out = {}
    for fl in man["files"]:
        ev = L.Events(L.Annotation(fl["interval"], fl["map"]), ("SHORT_READ",), (fl["R"],))
        ctx = L.Context(0)
        for k, v in man["options"].items():
            ctx.set_option(k, v)
        ctx.upload_events(ev)
        ctx.upload_reads(0, L.Reads.from_mrf(fl["mrf"], ev))
        res = out[fl["name"]] = {}
        for grid in fl["grids"]:
            if grid is None:
                os.environ.pop("LSQ_GRID_WGS", None)
            else:
                os.environ["LSQ_GRID_WGS"] = str(grid)
            for mode in fl["modes"]:
                os.environ["LSQ_ABLATE"] = str(mode)
                ctx.count()
                cnt, bases = ctx.counts()
                exc, rec = ctx.count_status()
                compact, _, pool = ctx.pool_format(0)
                res["%s/%d" % (grid, mode)] = {
                    "cnt": [int(x) for x in cnt[0]], "bases": [int(x) for x in bases[0]], "dbg": ctx.debug_counters(),
                    "exceptions": int(exc[0]), "recounted": int(rec[0]), "reads_per_look": ctx.launch_info()[0],
                    "compact": bool(compact), "pool": list(pool)}
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
