# Patch for tools/build_patched.sh (experiment record, r07): the persistent list kernel's batches
# without the two register-pressure measures on scatter_at's loop invariants (OPQ: the light count
# opaque at gen_index, 1 / n_lights passed in an SGPR pair). The compiler then hoists gen_index's
# rejection zone and its 64-bit operand into two VGPR pairs held through the render loop and spills
# them (4 VGPRs, 32 B of scratch per lane, reloaded only on the more-than-two-lights path); SGPR
# spills and the loop's lane read/write sites stay at the parent's 16 and 35. Same box, cornell
# 800x800x256: 21.35-21.60 ms against 21.47-21.51 ms for the tree (profiles/r07_ab_regalloc_variants.log):
# no difference beyond the spread, so the tree keeps the form without a private segment.
import sys
p = sys.argv[1]
s = open(p).read()
def rep(old, new):
    global s
    assert s.count(old) == 1, old[:100]
    s = s.replace(old, new, 1)
rep('''scatter_at<EXT, STATS, !HAS_MESH, PRIM>(S, mp, g,''', '''scatter_at<EXT, STATS, !HAS_MESH, false>(S, mp, g,''')
open(p, 'w').write(s)
