"""dbat_amd -- MI355X-native damped bundle adjustment behind DBAT's bundle() API.

Host-side mirror of the reference's interface for the bundle hot path:
    dbatstruct   the DBAT struct (prob2dbatstruct.m field layout)
    driver       bundle(s, ...) -> (s, ok, iters, sigma0, E); bundle_cov(s, E, 'CIO','CEO','COP');
                 bundle_reliability(s, E): redundancy numbers, standardized residuals, blunder suspects
                 ray_angles(s, E): intersection angles of every object point and every image, ray counts
                 point_depths(s, E): depth of every object point in every camera that sees it (the chirality veto's test)
                 network_quality(s, E): image coverage and marking-residual statistics, on the device
                 rigidalign, multixform, multialign: misc/rigidalign.m, pm_multixform.m, pm_multialign.m on the device;
                 transform_network(s, T), align_network(s, ref_OP): a whole struct into another coordinate system
    loadpm       PhotoModeler export loader (known-answer fixtures)
    initial      resect / forwintersect: initial EO and OP (photogrammetry/resect.m, forwintersect.m);
                 essmat5 / camsfrome / relorient / relorient_pairs: relative orientation of image pairs by a five-point
                 RANSAC (photogrammetry/essmat5.m, camsfrome.m), for networks without control points or EO
    report       the result file (bundle_result_file.m)
    diagnose     post-mortem of rank-deficient problems (bundle.m:368-446)
    parallel     torch.distributed / RCCL plumbing for sharded object points
    _hip         ctypes binding of include/dbat_hip.h (libdbat_hip.so)
"""
from .dbatstruct import make_struct, seteoest_depend, validate  # noqa: F401
from .driver import bundle, bundle_cov, bundle_reliability, ray_angles, point_depths, network_quality, BadInput  # noqa: F401
from .driver import rigidalign, multixform, multialign, transform_network, align_network  # noqa: F401
