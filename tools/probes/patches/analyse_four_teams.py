"""Timing experiment (results wrong by construction): kAnalyseTeams with FOUR teams of 256 threads per workgroup -- the fourth team
shares the first one's transform buffer (there is no LDS for a fourth beside the full tables) -- to see what sixteen waves per CU at a
128-register budget would buy before building the lean-table form that would make it legal.  Run the bench with --no-self-check."""
import sys
p = sys.argv[1] + '/smst_kernels.hip'
s = open(p).read()
def rep(old, new, count=1):
    global s
    assert s.count(old) == count, (s.count(old), old)
    s = s.replace(old, new)
# TeamWorkgroup carves the LDS for all three team kernels: at most three transform buffers, whatever TEAMS says (the others have two or three teams)
rep("lds = reinterpret_cast<float2 *>(twB + 8*R3) + (size_t)team*(H + H/16);", "lds = reinterpret_cast<float2 *>(twB + 8*R3) + (size_t)(team % 3)*(H + H/16);")
rep("(size_t)TEAMS*(H + H/16));", "(size_t)(TEAMS < 3 ? TEAMS : 3)*(H + H/16));")
rep("hipLaunchKernelGGL((kAnalyseTeams<r3.value, 3, exact.value>), dim3(teamsWorkgroups(d, jobs)), dim3(768), teamLdsBytes(d.M, 3)",
    "hipLaunchKernelGGL((kAnalyseTeams<r3.value, 4, exact.value>), dim3(teamsWorkgroups(d, jobs)), dim3(1024), teamLdsBytes(d.M, 3)")
open(p, 'w').write(s)
