"""sodt_detect_fwd and sodt_detect_bwd alone at the benchmark shape (B = 8, HW = 256^2, K = 128, na = 3, no = 13), three launches
each on random operands: the workload of a counter pass,
  rocprofv3 --pmc <counters> --output-format csv -d <dir> -- python tools/detect_once.py
(counters in a run of their own, no tracing beside them)."""
import importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
ops = importlib.import_module(bench.PKG + ".ops")


def main():
    dev = torch.device("cuda:0")
    B, HW, K, na, no = 8, 256 * 256, 128, 3, 13
    M, N = B * HW, na * no
    X = torch.randn(M, K, device=dev).bfloat16()
    W = torch.zeros(48, K, device=dev, dtype=torch.bfloat16)
    W[:N] = (torch.randn(N, K, device=dev) / K ** 0.5).bfloat16()
    bias = torch.randn(N, device=dev)
    pred = torch.empty(B, na, HW, no, device=dev)
    dX = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
    dW, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    ops.set_tn_scratch(torch.empty(16 << 20, device=dev))
    for _ in range(3):
        assert ops.detect_fwd(X, W, bias, pred, B, HW, na, no, K)
        assert ops.detect_bwd(pred, X, W, dX, dW, db, B, HW, na, no, K)
    torch.cuda.synchronize()
    print("pred", float(pred.abs().max()), "dX", float(dX.float().abs().max()), "dW", float(dW.abs().max()))


if __name__ == "__main__":
    main()
