"""Timing experiment (results wrong by construction): the plain record takes the parked previous-hop value AS the finished twist TW
(no Q, no two complex products, no rotation factor), and the line-aligned producers of kVocoder no longer fetch the two rotation
factors per lane and block.  What the recurrence kernel would cost if the analysis pass delivered TW in Xprev -- an upper bound of
that product, whose analysis pass gets heavier.  EXPERIMENTS.md, "The previous-hop twist formed once per bin" (priced with this, then built).
usage: tools/probes/build_variant.sh twistprice --git db89a58 tools/probes/patches/voc_twist_pricing.py   (the patch addresses the record as it
was before the twisted form existed)"""
import sys
d = sys.argv[1]
p = d + '/smst_vocoder_common.h'
s = open(p).read()
old = ("		const float2 rotB = rotate ? v.rot(off) : make_float2(1.f, 0.f);\n"
       "		const float2 Q = cmul(v.prev(mc, off), rotB);\n"
       "		const float2 Px = v.in(mc, off);\n"
       "		const float2 TW = cmul(rotB, cmulc(Px, Q));\n")
new = ("		const float2 Px = v.in(mc, off);\n"
       "		const float2 TW = v.prev(mc, off);\n")
assert s.count(old) == 1
open(p, 'w').write(s.replace(old, new))
# vocoderProduceAligned (smst_vocoder.hip comes before smst_vocoder_cont.hip in the joined file: the FIRST occurrence of each line)
p = d + '/smst_kernels.hip'
s = open(p).read()
for old in ("		asyncLoad8(rotNext1, d.rot + min(max(b + 1, 0), M - 1));\n",
            "		asyncLoad8(rotNextL, d.rot + min(max(b + L, 0), M - 1));\n",
            "		asyncArrived(rotNext1);\n",
            "		asyncArrived(rotNextL);\n",
            "		rot1 = asyncValue(rotNext1);\n",
            "		rotL = asyncValue(rotNextL);\n"):
    at = s.index(old)
    assert at < s.index("asyncLoad8(rotNext1, d.rot + min(b + 1, M - 1));"), old  # (kVocoderCont's own request)
    s = s[:at] + s[at + len(old):]
open(p, 'w').write(s)
