"""k_render_layers_dp_grad mutant (profiles/render_dp_grad/mutants.txt): the last workgroup does not write its row of partial."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    '    block_sum_store<3>(acc, e.partial + (int64_t)blockIdx.x * 3);',
    '    if (blockIdx.x + 1 < gridDim.x) block_sum_store<3>(acc, e.partial + (int64_t)blockIdx.x * 3);')
