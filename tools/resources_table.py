"""The resources table of every kernel of a build (profiles/*_resources_*.tsv) from the compiler's remarks.
usage: EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage bash csrc/build.sh 2> build.log; python tools/resources_table.py build.log > table.tsv
Names are demangled with c++filt (llvm-cxxfilt) when one is on the PATH."""
import re, shutil, subprocess, sys

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch_bytes_per_lane"),
          ("LDS Size [bytes/block]", "lds_bytes"), ("Occupancy [waves/SIMD]", "occupancy_waves_per_simd"))
rows, cur = {}, {}                                                      # (cur per source: a side-by-side build interleaves the files' remarks)
for line in open(sys.argv[1], errors="replace"):
    m = (re.match(r"(\S+?):\d+:\d+: remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line) or
         re.match(r"remark: (\S+?):\d+:\d+:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line))   # (newer compilers put the word first)
    if not m:
        continue
    src, text = m.groups()
    if text.startswith("Function Name: "):
        cur[src] = rows.setdefault((src, text[len("Function Name: "):]), {})
    elif src in cur:
        key, _, val = text.rpartition(": ")
        cur[src][key.strip()] = val
names = sorted({k[1] for k in rows})
filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if filt and names else names
ANON = "(anonymous namespace)::"
plain = dict(zip(names, (re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", p).replace(ANON, "\0")).replace("\0", ANON) for p in plain)))
print("file\tkernel\t" + "\t".join(f[1] for f in FIELDS))
for (src, name), r in sorted(rows.items(), key=lambda kv: (kv[0][0], plain[kv[0][1]])):
    print(src + "\t" + plain[name] + "\t" + "\t".join(r.get(f[0], "") for f in FIELDS))
