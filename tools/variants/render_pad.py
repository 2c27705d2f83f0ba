"""A/B of the wave-per-pixel renderers (k_local_psf_render_wave / k_psfnet_render_wave share render_wave):
patch rows padded by one position -- the last tap of a kernel row and the first of the next then fall into different LDS banks
(84 - 20 = 64 eight-byte words apart today: the same bank pair; SQ_LDS_BANK_CONFLICT = 47 % of SQ_LDS_IDX_ACTIVE,
profiles/r06/summary_render.json)."""
import sys
from _edit import sub
root = sys.argv[1]
sub(root, "sdirt_render.hip", "    static constexpr int NPOS = KS * PW;                    // patch positions",
    "    static constexpr int NPOS = KS * PW;                    // patch positions\n    static constexpr int PWS = PW + 1;                      // row stride in LDS")
sub(root, "sdirt_render.hip", "lds_bytes = (size_t)NPOS * 4 * sizeof(", "lds_bytes = (size_t)KS * PWS * 4 * sizeof(")
sub(root, "sdirt_render.hip", "        ptap[it] = (KS - 1 - fi) * PW + (KS - 1 - fj);", "        ptap[it] = (KS - 1 - fi) * G::PWS + (KS - 1 - fj);")
sub(root, "sdirt_render.hip", "                patch[e] = v;", "                patch[r * G::PWS + (e - r * PW)] = v;")
