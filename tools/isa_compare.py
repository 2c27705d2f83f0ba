"""Compare the gfx950 ISA of the kernels whose name contains a pattern between two compiles of one translation unit:
    python tools/isa_compare.py OLD.s NEW.s k_trace
(the .s files the Makefile leaves in sdirt_amd/csrc/obj).  Comments are dropped and the numbering of local labels is
ignored (it shifts when a kernel is added to the file); every instruction and operand must be equal.  Exit status 1
when a kernel differs or is missing."""
import re,sys
def kernels(path):
    out={}; name=None; buf=[]
    for line in open(path):
        m=re.match(r'^(_Z\w+):\s', line)
        if m: name=m.group(1); buf=[]; continue
        if name is not None:
            if line.startswith('.Lfunc_end'):
                out[name]=buf; name=None; continue
            l=re.sub(r'\.L(BB|tmp|func_begin|JTI)\d+_', r'.L\1_', line.split(';')[0].rstrip())
            if l.strip(): buf.append(l)
    return out
a=kernels(sys.argv[1]); b=kernels(sys.argv[2]); pat=sys.argv[3]
n=0
for k in a:
    if pat in k:
        n+=1
        print(k[:90], len(a[k]), 'SAME' if a[k]==b.get(k) else 'DIFF' if k in b else 'MISSING')
print(n, 'kernels')
sys.exit(0 if n and all(a[k] == b.get(k) for k in a if pat in k) else 1)
