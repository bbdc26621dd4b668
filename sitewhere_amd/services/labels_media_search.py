"""service-label-generation, service-streaming-media and service-event-search (multitenant).

* label generation -- ``QrCodeGenerator.java:37-70``; RPCs (``label-generation.proto``, 10):
  Get{CustomerType,Customer,AreaType,Area,DeviceType,Device,DeviceGroup,DeviceAssignment,AssetType,Asset}Label
* streaming media -- ``DeviceStreamManager.java:36``: stream creation acks and chunked stream data
  (sequence numbers), data requests answered from storage
* event search -- ``SearchProviderManager`` + ``SolrSearchProvider.java:51``: external search providers
  (Solr over HTTP) and an in-process provider over the tenant's event store
"""
from __future__ import annotations

import json
import urllib.parse
import urllib.request

from ..core.errors import ErrorCode, NotFoundException, SiteWhereSystemException
from ..models.domain import DeviceStreamData, Label, SearchResults, now_ms
from ..persistence.store import create_store
from ..runtime.microservice import MicroserviceTenantEngine, MultitenantMicroservice
from .qrcode import QrCode


# ============================================================================ labels
class LabelGeneration:
    ENTITIES = {
        "customer_type": ("DeviceManagement", "get_customer_type", "customertype"),
        "customer": ("DeviceManagement", "get_customer", "customer"),
        "area_type": ("DeviceManagement", "get_area_type", "areatype"),
        "area": ("DeviceManagement", "get_area", "area"),
        "device_type": ("DeviceManagement", "get_device_type", "devicetype"),
        "device": ("DeviceManagement", "get_device", "device"),
        "device_group": ("DeviceManagement", "get_device_group", "devicegroup"),
        "device_assignment": ("DeviceManagement", "get_device_assignment", "assignment"),
        "asset_type": ("AssetManagement", "get_asset_type", "assettype"),
        "asset": ("AssetManagement", "get_asset", "asset"),
    }

    def __init__(self, engine, generators: dict):
        self._e = engine
        self._gens = generators

    def _label(self, kind: str, generator_id: str, entity_id: str) -> Label:
        g = self._gens.get(generator_id)
        if g is None:
            raise NotFoundException(ErrorCode.Error, f"label generator {generator_id}")
        svc, getter, path = self.ENTITIES[kind]
        ent = getattr(self._e.ms.api(svc, self._e.tenant.token), getter)(entity_id)
        if ent is None:
            raise NotFoundException(ErrorCode.Error, f"{kind} {entity_id}")
        url = g.get("baseUrl", "sitewhere://{tenant}/{path}/{token}").format(
            tenant=self._e.tenant.token, path=path, token=getattr(ent, "token", None) or ent.id)
        qr = QrCode(url, ec=g.get("ecLevel", "M"))
        return Label("image/png", qr.to_png(int(g.get("scale", 6))))

    def get_customer_type_label(self, g, i): return self._label("customer_type", g, i)
    def get_customer_label(self, g, i): return self._label("customer", g, i)
    def get_area_type_label(self, g, i): return self._label("area_type", g, i)
    def get_area_label(self, g, i): return self._label("area", g, i)
    def get_device_type_label(self, g, i): return self._label("device_type", g, i)
    def get_device_label(self, g, i): return self._label("device", g, i)
    def get_device_group_label(self, g, i): return self._label("device_group", g, i)
    def get_device_assignment_label(self, g, i): return self._label("device_assignment", g, i)
    def get_asset_type_label(self, g, i): return self._label("asset_type", g, i)
    def get_asset_label(self, g, i): return self._label("asset", g, i)

    def list_label_generators(self) -> list[dict]:
        return [{"id": k, **v} for k, v in self._gens.items()]


class LabelGenerationTenantEngine(MicroserviceTenantEngine):
    def tenant_initialize(self, monitor):
        gens = {g["id"]: g for g in self.config.get("generators", [{"id": "qrcode", "type": "qrcode"}])}
        self.api = {"LabelGeneration": LabelGeneration(self, gens)}


class LabelGenerationMicroservice(MultitenantMicroservice):
    identifier = "label-generation"
    name = "Label Generation"

    def service_names(self):
        return ["LabelGeneration"]

    def create_tenant_engine(self, tenant):
        return LabelGenerationTenantEngine(self, tenant)


# ============================================================================ streaming media
class DeviceStreamManager:
    """Stream data chunks per (assignment, stream), reassembled in sequence order
    (``DeviceStreamManager.java``).  Chunks live in the tenant's configured datastore (memory, SQLite,
    MongoDB...; the reference's Mongo / Cassandra stream stores throw "not supported"), keyed by
    (assignment, stream, sequence number) so a re-sent chunk replaces itself."""

    COLLECTION = "deviceStreamData"

    def __init__(self, engine, store=None):
        self._e = engine
        self._store = store or create_store("memory")
        self._store.register(self.COLLECTION, DeviceStreamData, ())

    def _dm(self):
        return self._e.ms.api("DeviceManagement", self._e.tenant.token)

    def handle_device_stream_request(self, device_token: str, request: dict) -> dict:
        dm = self._dm()
        dev = dm.get_device_by_token(device_token)
        if dev is None or not dev.device_assignment_id:
            return {"streamId": request.get("streamId"), "state": "STREAM_FAILED"}
        if dm.get_device_stream_by_stream_id(dev.device_assignment_id, request["streamId"]):
            return {"streamId": request["streamId"], "state": "STREAM_EXISTS"}
        dm.create_device_stream(dev.device_assignment_id, {"streamId": request["streamId"],
                                                           "contentType": request.get("contentType", ""),
                                                           "metadata": request.get("metadata", {})})
        return {"streamId": request["streamId"], "state": "STREAM_CREATED"}

    @staticmethod
    def _key(assignment_id: str, stream_id: str, seq: int) -> str:
        return f"{assignment_id}:{stream_id}:{int(seq)}"

    def add_device_stream_data(self, assignment_id: str, stream_id: str, sequence_number: int, data: bytes,
                               event_date: int | None = None) -> DeviceStreamData:
        if self._dm().get_device_stream_by_stream_id(assignment_id, stream_id) is None:
            raise SiteWhereSystemException(ErrorCode.InvalidStreamId, detail=stream_id)
        d = DeviceStreamData(id=self._key(assignment_id, stream_id, sequence_number),
                             device_assignment_id=assignment_id, stream_id=stream_id,
                             sequence_number=int(sequence_number), data=bytes(data),
                             event_date=event_date or now_ms(), received_date=now_ms())
        return self._store.put(self.COLLECTION, d)

    def get_device_stream_data(self, assignment_id: str, stream_id: str, sequence_number: int):
        return self._store.get(self.COLLECTION, self._key(assignment_id, stream_id, sequence_number))

    def list_device_stream_data(self, assignment_id: str, stream_id: str) -> SearchResults:
        chunks = self._store.query(self.COLLECTION, lambda d: d.device_assignment_id == assignment_id and
                                   d.stream_id == stream_id, sort_key=lambda d: d.sequence_number)
        return SearchResults(len(chunks), chunks)

    def get_stream_content(self, assignment_id: str, stream_id: str) -> bytes:
        return b"".join(d.data for d in self.list_device_stream_data(assignment_id, stream_id).results)


class StreamingMediaTenantEngine(MicroserviceTenantEngine):
    def tenant_initialize(self, monitor):
        ds = self.config.get("datastore", {"type": "memory"})
        store = create_store(ds.get("type", "memory"), **{k: v for k, v in ds.items() if k != "type"})
        self.api = {"StreamingMedia": DeviceStreamManager(self, store)}


class StreamingMediaMicroservice(MultitenantMicroservice):
    identifier = "streaming-media"
    name = "Streaming Media"

    def service_names(self):
        return ["StreamingMedia"]

    def create_tenant_engine(self, tenant):
        return StreamingMediaTenantEngine(self, tenant)


# ============================================================================ event search
class SolrSearchProvider:
    def __init__(self, pid: str, url: str, collection: str = "SiteWhere", get=None):
        self.pid, self.url, self.collection = pid, url.rstrip("/"), collection
        self._get = get

    def search(self, query: str, rows: int = 100) -> list[dict]:
        url = f"{self.url}/{self.collection}/select?{urllib.parse.urlencode({'q': query, 'rows': rows, 'wt': 'json'})}"
        body = self._get(url) if self._get else urllib.request.urlopen(url, timeout=10).read()
        return json.loads(body).get("response", {}).get("docs", [])

    def get_locations_near(self, latitude: float, longitude: float, distance: float, criteria=None) -> dict:
        """No geospatial query is sent to Solr: an empty result, as ``SolrSearchProvider.getLocationsNear``
        of the reference answers."""
        return {"hotSince": None, "numResults": 0, "results": [], "distances": []}

    def get_locations_in_zone(self, zone_token: str, criteria=None) -> dict:
        """No geospatial query is sent to Solr: an empty result, as for :meth:`get_locations_near`."""
        return {"hotSince": None, "numResults": 0, "results": []}

    def get_locations_grid(self, criteria=None) -> dict:
        """No geospatial query is sent to Solr: an empty grid, as for :meth:`get_locations_near`."""
        from ..pipeline.grid import check_grid_args, grid_steps
        c = criteria or {}
        box, rows, cols = check_grid_args(c.get("latMin"), c.get("latMax"), c.get("lonMin"), c.get("lonMax"),
                                          c.get("rows"), c.get("cols"), c.get("startDate"), c.get("endDate"))
        d_lat, d_lon, _ = grid_steps(box, rows, cols)
        return {"hotSince": None, "numResults": 0, "outside": 0, "invalid": 0, "rows": rows, "cols": cols,
                "latStep": d_lat, "lonStep": d_lon, "cells": []}

    def get_event_ranking(self, criteria=None) -> dict:
        """No aggregation is sent to Solr: an empty ranking, once the arguments are checked."""
        _rank_criteria(criteria)
        return {"hotSince": None, "numResults": 0, "nan": 0, "ungrouped": 0, "groups": 0, "results": []}


_RANK_TYPES = {"Measurement": 0, "Location": 1, "Alert": 2, "StateChange": 5}    # EV_* of models/columnar.py
_RANK_LISTS = {"Measurement": "list_measurements_for_index", "Location": "list_locations_for_index",
               "Alert": "list_alerts_for_index", "StateChange": "list_state_changes_for_index"}


def _rank_criteria(criteria):
    """The ranking criteria, checked (``pipeline/rank.py: check_rank_args``): a dict of the keyword arguments of
    ``GpuInboundApi.event_ranking_hot``."""
    from ..pipeline.rank import check_rank_args
    c = criteria or {}
    et, group = c.get("eventType"), c.get("groupBy")
    if et not in _RANK_TYPES or group not in ("Assignment", "Customer", "Area", "Asset"):
        raise ValueError("eventType must be Measurement, Location, Alert or StateChange and groupBy Assignment, "
                         "Customer, Area or Asset")
    mx, al = c.get("measurementId"), c.get("alertType")
    if (mx is not None and et != "Measurement") or (al is not None and et != "Alert"):
        raise ValueError("measurementId is for measurements and alertType for alerts")
    name = mx if et == "Measurement" else al
    args = dict(event_type=et, group_by=group, stat=c.get("stat") or "count", top=c.get("top", 10), measurement_id=mx,
                alert_type=al, min_level=c.get("minLevel"), start_date=c.get("startDate"), end_date=c.get("endDate"),
                ascending=bool(c.get("ascending", False)))
    check_rank_args(_RANK_TYPES[et], group.lower(), args["stat"], args["top"], args["start_date"], args["end_date"],
                    None if name is None else 0, args["min_level"])
    return args


class EventStoreSearchProvider:
    """In-process provider: ``field:value`` terms (AND) over the tenant's event store."""

    def __init__(self, pid: str, engine):
        self.pid, self._e = pid, engine

    def search(self, query: str, rows: int = 100) -> list[dict]:
        terms = dict(t.split(":", 1) for t in query.split() if ":" in t)
        em = self._e.ms.api("DeviceEventManagement", self._e.tenant.token)
        from ..models.domain import DateRangeSearchCriteria, DeviceEventType
        et = DeviceEventType(terms.pop("eventType", "Measurement"))
        idx = "Assignment"
        ids = []
        for k in ("assignment", "customer", "area", "asset"):
            if k in terms:
                idx, ids = k.title(), [terms.pop(k)]
        fn = {DeviceEventType.Measurement: em.list_measurements_for_index, DeviceEventType.Location: em.list_locations_for_index,
              DeviceEventType.Alert: em.list_alerts_for_index}.get(et, em.list_measurements_for_index)
        res = fn(idx, ids, DateRangeSearchCriteria(page_size=rows))
        out = []
        for ev in res.results:
            d = ev.to_dict()
            if all(str(d.get(k)) == v for k, v in terms.items()):
                out.append(d)
        return out

    def get_locations_near(self, latitude: float, longitude: float, distance: float, criteria=None) -> dict:
        """``IDeviceEventSearchProvider.getLocationsNear``: the tenant's locations within ``distance``
        metres of a point.  ``criteria``: a date-range criteria object or a dict (``startDate``,
        ``endDate``, ``pageNumber``, ``pageSize``, and the additions ``latest`` and ``order``).  Served
        from the inbound engine's event ring when the tenant has one and the ring covers the range --
        it has not wrapped, or ``startDate >= hotSince`` -- else from event management's list of the
        range's locations, filtered on the host by the same function (``pipeline/near.py``).  Returns
        ``{"hotSince", "numResults", "results", "distances"}`` on both routes; ``ValueError`` for a
        point or a distance out of range."""
        from ..pipeline.near import check_near_args, host_near
        c = criteria or {}
        if not isinstance(c, dict):
            c = {"startDate": c.start_date, "endDate": c.end_date, "pageNumber": c.page_number, "pageSize": c.page_size}
        start, end = c.get("startDate"), c.get("endDate")
        latest, order = bool(c.get("latest", False)), c.get("order") or "date"
        page, size = int(c.get("pageNumber") or 1), int(c.get("pageSize", 100))
        check_near_args(latitude, longitude, distance, start, end, order)
        token = self._e.tenant.token
        hot = self._e.ms.api("InboundProcessing", token).locations_near_hot(
            latitude, longitude, distance, start, end, None, None, latest, order, page, size)
        if hot is not None and (hot["hotSince"] is None or (start is not None and start >= hot["hotSince"])):
            return hot
        asgs = self._e.ms.api("DeviceManagement", token).list_device_assignments({"pageNumber": 1, "pageSize": 0})
        locs = self._e.ms.api("DeviceEventManagement", token).list_locations_for_index(
            "Assignment", [a.id for a in asgs.results],
            {"pageNumber": 1, "pageSize": 0, "startDate": start, "endDate": end}).results
        return host_near(locs, latitude, longitude, distance, start, end, latest, order, page, size)

    def get_locations_in_zone(self, zone_token: str, criteria=None) -> dict:
        """The tenant's locations inside a zone (``Zone.bounds`` as a planar (lat, lon) polygon, the
        test ``core/geo.contains``).  ``criteria``: a date-range criteria object or a dict (``startDate``,
        ``endDate``, ``pageNumber``, ``pageSize``, and the additions ``outside``: the locations outside
        the zone, and ``latest``: only each assignment's newest location in the range is looked at).
        Served from the inbound engine's event ring when the tenant has one and the ring covers the
        range, by :meth:`get_locations_near`'s rule, else from event management's list of the range's
        locations, filtered on the host by the same function (``pipeline/zone.py``); a zone of more
        than ``ZONE_MAX_VTX`` bounds always takes the host route.  Returns ``{"hotSince", "numResults",
        "results"}``, newest first.  An unknown zone is not found; ``ValueError`` for a zone of fewer
        than 3 bounds or ``startDate > endDate``."""
        from ..core.geo import polygon_of
        from ..pipeline.zone import ZONE_MAX_VTX, check_zone_args, host_zone
        c = criteria or {}
        if not isinstance(c, dict):
            c = {"startDate": c.start_date, "endDate": c.end_date, "pageNumber": c.page_number, "pageSize": c.page_size}
        start, end = c.get("startDate"), c.get("endDate")
        outside, latest = bool(c.get("outside", False)), bool(c.get("latest", False))
        page, size = int(c.get("pageNumber") or 1), int(c.get("pageSize", 100))
        token = self._e.tenant.token
        zone = self._e.ms.api("DeviceManagement", token).get_zone_by_token(zone_token)
        if zone is None:
            raise NotFoundException(ErrorCode.Error, f"zone {zone_token}")
        poly = check_zone_args(polygon_of(zone.bounds or []), start, end, max_vtx=None)
        if len(poly) <= ZONE_MAX_VTX:
            hot = self._e.ms.api("InboundProcessing", token).locations_in_zone_hot(
                poly, start, end, None, None, outside, latest, page, size)
            if hot is not None and (hot["hotSince"] is None or (start is not None and start >= hot["hotSince"])):
                return hot
        asgs = self._e.ms.api("DeviceManagement", token).list_device_assignments({"pageNumber": 1, "pageSize": 0})
        locs = self._e.ms.api("DeviceEventManagement", token).list_locations_for_index(
            "Assignment", [a.id for a in asgs.results],
            {"pageNumber": 1, "pageSize": 0, "startDate": start, "endDate": end}).results
        return host_zone(locs, poly, start, end, outside, latest, page, size)

    def get_locations_grid(self, criteria=None) -> dict:
        """A density grid of the tenant's locations over a lat/lon box (``EngineBase.grid_store`` has the
        contract).  ``criteria``: a dict of ``latMin``, ``latMax``, ``lonMin``, ``lonMax`` (``lonMin >
        lonMax``: the box crosses the antimeridian), ``rows``, ``cols``, and optionally ``startDate``,
        ``endDate`` and ``latest`` (only each assignment's newest location in the range is looked at).
        Served from the inbound engine's event ring when the tenant has one and the ring covers the range,
        by :meth:`get_locations_near`'s rule, else from event management's list of the range's locations,
        counted on the host by the same function (``pipeline/grid.py``).  Returns ``{"hotSince",
        "numResults", "outside", "invalid", "rows", "cols", "latStep", "lonStep", "cells"}`` on both
        routes, ``cells`` the non-empty ones as ``{"row", "col", "count", "lastDate"}`` in row-major
        order; ``ValueError`` for a box or cell counts out of range or ``startDate > endDate``."""
        from ..pipeline.grid import check_grid_args, host_grid
        c = criteria or {}
        start, end, latest = c.get("startDate"), c.get("endDate"), bool(c.get("latest", False))
        box, rows, cols = check_grid_args(c.get("latMin"), c.get("latMax"), c.get("lonMin"), c.get("lonMax"),
                                          c.get("rows"), c.get("cols"), start, end)
        token = self._e.tenant.token
        hot = self._e.ms.api("InboundProcessing", token).locations_grid_hot(box, rows, cols, start, end, None, None, latest)
        if hot is not None and (hot["hotSince"] is None or (start is not None and start >= hot["hotSince"])):
            return hot
        asgs = self._e.ms.api("DeviceManagement", token).list_device_assignments({"pageNumber": 1, "pageSize": 0})
        locs = self._e.ms.api("DeviceEventManagement", token).list_locations_for_index(
            "Assignment", [a.id for a in asgs.results],
            {"pageNumber": 1, "pageSize": 0, "startDate": start, "endDate": end}).results
        return host_grid(locs, *box, rows, cols, start, end, latest)

    def get_event_ranking(self, criteria=None) -> dict:
        """The tenant's assignments, customers, areas or assets ranked by a statistic of their events
        (``EngineBase.rank_store`` has the contract).  ``criteria``: a dict of ``eventType`` (``Measurement``,
        ``Location``, ``Alert``, ``StateChange``), ``groupBy`` (``Assignment``, ``Customer``, ``Area``,
        ``Asset``) and optionally ``stat`` (``count``; ``min``, ``max``, ``last`` of ``measurementId``),
        ``top`` (None: every group), ``measurementId``, ``alertType``, ``minLevel``, ``startDate``,
        ``endDate`` and ``ascending``.  Served from the inbound engine's event ring when the tenant has one
        and the ring covers the range, by :meth:`get_locations_grid`'s rule, else from event management's
        list of the range's events, ranked on the host by the same function (``pipeline/rank.py``).
        Returns ``{"hotSince", "numResults", "nan", "ungrouped", "groups", "results"}`` on both routes;
        ``ValueError`` for arguments out of range or ``startDate > endDate``."""
        from ..pipeline.rank import host_rank
        a = _rank_criteria(criteria)
        start, end = a["start_date"], a["end_date"]
        token = self._e.tenant.token
        hot = self._e.ms.api("InboundProcessing", token).event_ranking_hot(**a)
        if hot is not None and (hot["hotSince"] is None or (start is not None and start >= hot["hotSince"])):
            return hot
        asgs = self._e.ms.api("DeviceManagement", token).list_device_assignments({"pageNumber": 1, "pageSize": 0})
        lister = getattr(self._e.ms.api("DeviceEventManagement", token), _RANK_LISTS[a["event_type"]])
        evs = lister("Assignment", [x.id for x in asgs.results],
                     {"pageNumber": 1, "pageSize": 0, "startDate": start, "endDate": end}).results
        name = a["measurement_id"] if a["event_type"] == "Measurement" else a["alert_type"]
        return host_rank(evs, _RANK_TYPES[a["event_type"]], a["group_by"].lower(), a["stat"], a["top"], start, end, name,
                         a["min_level"], a["ascending"])


class SearchProviderManager:
    def __init__(self, providers: dict):
        self._p = providers

    def list_search_providers(self) -> list[dict]:
        return [{"id": k, "type": type(v).__name__} for k, v in self._p.items()]

    def search(self, provider_id: str, query: str, rows: int = 100) -> list[dict]:
        p = self._p.get(provider_id)
        if p is None:
            raise NotFoundException(ErrorCode.Error, f"search provider {provider_id}")
        return p.search(query, rows)

    def get_locations_near(self, provider_id: str, latitude: float, longitude: float, distance: float,
                           criteria=None) -> dict:
        """The search SPI's ``getLocationsNear`` on one provider (see the providers' methods)."""
        p = self._p.get(provider_id)
        if p is None:
            raise NotFoundException(ErrorCode.Error, f"search provider {provider_id}")
        return p.get_locations_near(latitude, longitude, distance, criteria)

    def get_locations_in_zone(self, provider_id: str, zone_token: str, criteria=None) -> dict:
        """Locations in a zone on one provider (see the providers' methods)."""
        p = self._p.get(provider_id)
        if p is None:
            raise NotFoundException(ErrorCode.Error, f"search provider {provider_id}")
        return p.get_locations_in_zone(zone_token, criteria)

    def get_locations_grid(self, provider_id: str, criteria=None) -> dict:
        """A location density grid on one provider (see the providers' methods)."""
        p = self._p.get(provider_id)
        if p is None:
            raise NotFoundException(ErrorCode.Error, f"search provider {provider_id}")
        return p.get_locations_grid(criteria)

    def get_event_ranking(self, provider_id: str, criteria=None) -> dict:
        """A ranking of groups by their events on one provider (see the providers' methods)."""
        p = self._p.get(provider_id)
        if p is None:
            raise NotFoundException(ErrorCode.Error, f"search provider {provider_id}")
        return p.get_event_ranking(criteria)


class EventSearchTenantEngine(MicroserviceTenantEngine):
    def tenant_initialize(self, monitor):
        prov = {"events": EventStoreSearchProvider("events", self)}
        for pc in self.config.get("providers", []):
            if pc.get("type") == "solr":
                prov[pc["id"]] = SolrSearchProvider(pc["id"], pc["url"], pc.get("collection", "SiteWhere"))
        self.api = {"EventSearch": SearchProviderManager(prov)}


class EventSearchMicroservice(MultitenantMicroservice):
    identifier = "event-search"
    name = "Event Search"

    def service_names(self):
        return ["EventSearch"]

    def create_tenant_engine(self, tenant):
        return EventSearchTenantEngine(self, tenant)
