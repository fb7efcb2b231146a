"""halo_amd — MI355X-native receive parse-and-checksum engine for halo's rx path.

The hot path (protocol.Parse* + GetCheckSum driven by engine.RxEthernet/RxIpv4) runs as
hand-written HIP kernels for gfx950 behind the C ABI in include/halo_rx.h; this package is
the thin Python host side over that ABI (ctypes). See DESIGN.md.
"""
from . import _lib  # noqa: F401  (raises if libhalo_rx.so is not built: no CPU fallback)
from ._lib import ACTION, ACTION_NAMES, RESULT_DTYPE, STATUS, STATUS_NAMES, NetIf, HaloError  # noqa: F401
from ._lib import EGRESS_PORT_DTYPE  # noqa: F401
from .arp import ArpTable  # noqa: F401
from .deliver import DeliverResult, deliver, deliver_host, port_map  # noqa: F401
from .kcp import KcpEmitResult, KcpIngestResult  # noqa: F401
from .dhcp import DhcpBuildResult, DhcpDecodeResult, DhcpServer  # noqa: F401
from .egress import EgressResult, egress_arp, egress_host, egress_masks, egress_switch  # noqa: F401
from .nat import NatTable  # noqa: F401
from .respond import RespondResult, build_replies, respond, respond_host, tcp_port_map  # noqa: F401  (adds ArpTable.encap_tx)
from .switch import Switch  # noqa: F401
from .pmflow import PortMappingFlowTable, forward_return_flows  # noqa: F401  (adds ArpTable.encap_via)
from .loopback import LoResult  # noqa: F401
from . import loopback  # noqa: F401

__all__ = ["PortMappingFlowTable", "forward_return_flows","ACTION", "ACTION_NAMES", "RESULT_DTYPE", "STATUS", "STATUS_NAMES", "NetIf", "HaloError", "ArpTable", "NatTable",
           "Switch", "EGRESS_PORT_DTYPE", "EgressResult", "egress_arp", "egress_host", "egress_masks", "egress_switch",
           "RespondResult", "build_replies", "respond", "respond_host", "tcp_port_map",
           "DeliverResult", "deliver", "deliver_host", "port_map",
           "KcpIngestResult", "KcpEmitResult", "kcp",
           "DhcpServer", "DhcpDecodeResult", "DhcpBuildResult", "dhcp", "LoResult", "loopback"]
