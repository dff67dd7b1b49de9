"""Two training steps of BEVEncoderTransformer(128, 4) at batch 2 x 200x200 (fp16 autocast + GradScaler + Adam):
the workload behind profiles/r07_deform_train_step_kernel_summary.txt, run under
`rocprofv3 --kernel-trace --stats -- python tools/deform_train_step.py`.  DeformableAttention takes the native node
(LSS_DEFORM_NATIVE=0: the torch composition)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.nn import functional as F

from lss2_multimodal_nu_amd import model_vovnet_transformer as mv

torch.manual_seed(0)
m = mv.BEVEncoderTransformer(128, 4).cuda().train()
opt = torch.optim.Adam(m.parameters(), 1e-4)
scaler = torch.amp.GradScaler("cuda")
x = torch.randn(2, 128, 200, 200, device="cuda")
target = (torch.rand(2, 4, 200, 200, device="cuda") > 0.7).float()
for _ in range(2):
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        seg, _ = m(x)
        loss = F.binary_cross_entropy_with_logits(seg.float(), target)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
torch.cuda.synchronize()
print("step ok loss %.5f" % float(loss.detach()))
