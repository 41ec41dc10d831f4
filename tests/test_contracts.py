"""Event / document contracts: envelope, 17 event schemas, routing keys, deterministic ids, the
Draft 2020-12 validator subset.

Parity: over the reference's schema files stored under tests/golden/reference_schemas, every generated schema is
compared field-by-field with the reference's own JSON Schema file (docs/schemas/events/*.json,
docs/schemas/documents/v1/*.json) and sample events are validated against BOTH -- the same
cross-check the reference's tests/test_integration_message_flow.py:23-70 does with its
FileSchemaProvider.  Id vectors are recomputed from the reference's documented derivations
(identifier_generator.py:26-68) with hashlib directly.
"""
from __future__ import annotations

import hashlib
import json
import uuid
from pathlib import Path

import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from copilot_for_consensus_amd.contracts import documents, events, ids
from copilot_for_consensus_amd.contracts.registry import SchemaProvider, create_schema_provider
from copilot_for_consensus_amd.contracts.validator import (SchemaRegistry, ValidationError, iter_errors,
                                                            validate_json, validate_or_raise)

REF = Path(__file__).parent / "golden" / "reference_schemas"

H16 = "0123456789abcdef"
H64 = "ab" * 32
TS = "2025-01-02T03:04:05Z"
CID = str(uuid.UUID(int=7))

SAMPLES = {
    "ArchiveIngested": dict(archive_id=H16, source_name="ietf-quic", source_type="rsync", source_url="rsync://x/y",
                            file_size_bytes=10, file_hash_sha256=H64, ingestion_started_at=TS,
                            ingestion_completed_at=TS),
    "ArchiveIngestionFailed": dict(source_name="s", source_type="http", source_url="http://x", error_message="boom",
                                   error_type="IOError", retry_count=0, ingestion_started_at=TS, failed_at=TS),
    "JSONParsed": dict(archive_id=H16, message_count=1, message_doc_ids=[H16], thread_count=1, thread_ids=[H16],
                       parsing_duration_seconds=0.5),
    "ParsingFailed": dict(archive_id=H16, error_message="e", error_type="t", messages_parsed_before_failure=0,
                          retry_count=1, failed_at=TS),
    "ChunksPrepared": dict(message_doc_ids=[H16], chunk_count=2, chunk_ids=[H16, "fedcba9876543210"], chunks_ready=True,
                           chunking_strategy="token_window", avg_chunk_size_tokens=300),
    "ChunkingFailed": dict(message_doc_ids=[H16], error_message="e", error_type="t", retry_count=0, failed_at=TS),
    "EmbeddingsGenerated": dict(chunk_ids=[H16], embedding_count=1, embedding_model="all-MiniLM-L6-v2",
                                embedding_backend="hip", embedding_dimension=384, vector_store_collection="message_embeddings",
                                vector_store_updated=True, avg_generation_time_ms=1.5),
    "EmbeddingGenerationFailed": dict(chunk_ids=["c1"], error_message="e", error_type="t", embedding_backend="hip",
                                      retry_count=0, failed_at=TS),
    "SummarizationRequested": dict(thread_ids=[H16], top_k=5, prompt_template="Summarize {email_chunks}",
                                   selected_chunks=[{"chunk_id": H16, "source": "thread", "score": 0.5, "rank": 0}],
                                   context_selection={"selector_type": "top_k_relevance", "selector_version": "1.0"}),
    "OrchestrationFailed": dict(thread_ids=[H16], error_type="t", error_message="e", retry_count=0),
    "SummaryComplete": dict(summary_id=H64, thread_id=H16, summary_markdown="# s", citations=[
        {"message_id": "<m@x>", "chunk_id": H16, "offset": 0, "text": "quote"}], llm_backend="hip",
        llm_model="mistral-7b", tokens_prompt=10, tokens_completion=5, latency_ms=100),
    "SummarizationFailed": dict(thread_id=H16, error_type="t", error_message="e", retry_count=0),
    "ReportPublished": dict(thread_id=H16, report_id=H16, format="markdown", notified=False, delivery_channels=[],
                            summary_url="/api/reports/x"),
    "ReportDeliveryFailed": dict(report_id=H16, thread_id=H16, delivery_channel="webhook", error_message="e",
                                 error_type="t", retry_count=0),
    "SourceDeletionRequested": dict(source_name="s", correlation_id=CID, requested_at=TS, archive_ids=[H16],
                                    delete_mode="hard"),
    "SourceCleanupProgress": dict(source_name="s", correlation_id=CID, service_name="chunking", status="completed",
                                  deletion_counts={"chunks": 3}),
    "SourceCleanupCompleted": dict(source_name="s", correlation_id=CID, completed_at=TS, total_deletion_counts={},
                                   services_completed=["parsing"], services_failed=[], overall_status="success"),
}


def sample_event(t):
    return events.Event(t, dict(SAMPLES[t])).to_dict()


def test_seventeen_event_types_and_routing_keys():
    assert len(events.EVENT_TYPES) == 17
    assert set(SAMPLES) == set(events.EVENT_TYPES)
    assert events.routing_key_for("JSONParsed") == "json.parsed"
    assert events.routing_key_for("ArchiveIngested") == "archive.ingested"
    assert events.routing_key_for("SummarizationRequested") == "summarization.requested"
    assert events.routing_key_for("EmbeddingGenerationFailed") == "embedding.generation.failed"
    assert len(set(events.ROUTING_KEYS.values())) == 17
    for t, k in events.ROUTING_KEYS.items():
        assert events.EVENT_FOR_ROUTING_KEY[k] == t


@pytest.mark.parametrize("etype", list(SAMPLES))
def test_sample_events_validate(etype):
    prov = SchemaProvider()
    ev = sample_event(etype)
    assert prov.validate_event(ev) == []
    assert events.Event.from_dict(json.loads(json.dumps(ev))) == events.Event.from_dict(ev)


@pytest.mark.parametrize("etype", list(SAMPLES))
def test_events_reject_missing_extra_and_wrong_type(etype):
    prov = SchemaProvider()
    req, _ = events.EVENT_SPECS[etype]
    ev = sample_event(etype)
    first = next(iter(req))
    bad = json.loads(json.dumps(ev))
    del bad["data"][first]
    assert prov.validate_event(bad), f"missing {first} accepted"
    bad = json.loads(json.dumps(ev))
    bad["data"]["unexpected_field"] = 1
    assert prov.validate_event(bad), "additionalProperties accepted"
    bad = json.loads(json.dumps(ev))
    bad["event_type"] = "Other" if etype != "JSONParsed" else "ChunksPrepared"
    assert prov.validate_event(bad)
    bad = json.loads(json.dumps(ev))
    bad["event_id"] = "not-a-uuid"
    assert prov.validate_event(bad)
    bad = json.loads(json.dumps(ev))
    del bad["timestamp"]
    assert prov.validate_event(bad)


def test_unknown_event_type_is_an_error():
    assert SchemaProvider().validate_event({"event_type": "Nope"})
    assert create_schema_provider().list_event_types() == list(events.EVENT_TYPES)


def _ref_data_schema(sch):
    for part in sch.get("allOf", []):
        d = part.get("properties", {}).get("data")
        if d:
            return d
    raise AssertionError("no data schema")


@pytest.mark.parametrize("etype", list(SAMPLES))
def test_event_schema_matches_reference_file(etype):
    ref = json.loads((REF / "events" / f"{etype}.schema.json").read_text())
    mine = events.event_schema(etype)
    assert mine["$id"] == ref["$id"]
    diffs = []
    _schema_diff(_ref_data_schema(mine), _ref_data_schema(ref), etype, diffs)
    assert diffs == []


_KW = ("type", "enum", "const", "pattern", "format", "minLength", "maxLength", "minimum", "maximum", "minItems",
       "maxItems", "uniqueItems", "additionalProperties", "required")


def _schema_diff(mine, ref, path, out):
    """Every assertion keyword of the reference schema, recursively through properties/items."""
    for k in _KW:
        if k in ref or k in mine:
            rv, mv = ref.get(k), mine.get(k)
            if k == "required":
                rv, mv = set(rv or []), set(mv or [])
            if rv != mv:
                out.append((path, k, mv, rv))
    for name, rp in ref.get("properties", {}).items():
        if name in mine.get("properties", {}):
            _schema_diff(mine["properties"][name], rp, f"{path}.{name}", out)
        else:
            out.append((path, "missing property", name))
    if "items" in ref and "items" in mine:
        _schema_diff(mine["items"], ref["items"], path + "[]", out)


def test_envelope_matches_reference_file():
    ref = json.loads((REF / "events" / "event-envelope.schema.json").read_text())
    diffs = []
    _schema_diff(events.envelope_schema(), ref, "envelope", diffs)
    assert diffs == []


@pytest.mark.parametrize("etype", list(SAMPLES))
def test_sample_events_validate_against_reference_schema_files(etype):
    reg = SchemaRegistry()
    env = json.loads((REF / "events" / "event-envelope.schema.json").read_text())
    reg.add(env, "event-envelope.schema.json", "./event-envelope.schema.json")
    ref = json.loads((REF / "events" / f"{etype}.schema.json").read_text())
    reg.add(ref, etype)
    ev = sample_event(etype)
    # the reference strips additionalProperties:false from allOf branches at validation time
    # (schema_validator.py _strip_allof_additional_properties); do the same for its files
    for part in ref.get("allOf", []):
        part.pop("additionalProperties", None)
    env.pop("additionalProperties", None)
    assert iter_errors(ev, ref, reg) == [], etype


@pytest.mark.parametrize("coll", ["archives", "messages", "threads", "chunks", "summaries", "sources"])
def test_document_schema_matches_reference_file(coll):
    ref = json.loads((REF / "documents" / "v1" / f"{coll}.schema.json").read_text())
    mine = documents.document_schema(coll)
    assert set(mine["required"]) == set(ref["required"]), coll
    missing = set(ref["properties"]) - set(mine["properties"])
    assert not missing, (coll, missing)


def test_document_schemas_accept_pipeline_documents():
    prov = SchemaProvider()
    arc = {"_id": H16, "file_hash": H64, "file_size_bytes": 1, "source": "s", "ingestion_date": TS, "status": "pending"}
    assert prov.validate_document("archives", arc) == []
    assert prov.validate_document("archives", {**arc, "status": "exploded"})
    chunk = {"_id": H16, "message_doc_id": H16, "message_id": "<a@b>", "thread_id": H16, "chunk_index": 0,
             "text": "t", "created_at": TS, "embedding_generated": False}
    assert prov.validate_document("chunks", chunk) == []
    assert prov.validate_document("chunks", {**chunk, "chunk_index": -1})


def test_schema_export_roundtrip(tmp_path):
    prov = SchemaProvider()
    paths = prov.export(tmp_path)
    assert len([p for p in paths if p.parent.name == "events"]) == 18
    for p in paths:
        json.loads(p.read_text())


# ------------------------------------------------------------------ deterministic ids
def test_ids_match_reference_derivations():
    data = b"From a@b Mon Jan  1 00:00:00 2024\nSubject: x\n\nhello\n"
    assert ids.archive_id_from_bytes(data) == hashlib.sha256(data).hexdigest()[:16]
    mid = ids.message_doc_id("arc", "<m@x>", "2024-01-01", "a@b", "Re: x")
    assert mid == hashlib.sha256(b"arc|<m@x>|2024-01-01|a@b|Re: x").hexdigest()[:16]
    # absent optional parts are skipped, not emptied
    assert ids.message_doc_id("arc", "<m@x>", None, "a@b") == hashlib.sha256(b"arc|<m@x>|a@b").hexdigest()[:16]
    assert ids.chunk_id(mid, 3) == hashlib.sha256(f"{mid}|3".encode()).hexdigest()[:16]
    sid = ids.summary_id("t1", ["c2", "c1"])
    assert sid == hashlib.sha256(b"t1:c1,c2").hexdigest() and len(sid) == 64
    assert ids.summary_id("t1", ["c1", "c2"]) == sid  # order independent
    assert ids.report_id(sid) == hashlib.sha256(sid.encode()).hexdigest()[:16]
    assert ids.content_summary_id("t", "md", TS) == hashlib.sha256(f"t|md|{TS}".encode()).hexdigest()[:16]


@settings(max_examples=200, deadline=None)
@given(st.text(max_size=40), st.text(max_size=40), st.lists(st.text(min_size=1, max_size=8), max_size=6))
def test_id_shapes(a, b, chunks):
    assert len(ids.message_doc_id(a, b)) == 16
    assert all(c in "0123456789abcdef" for c in ids.sha256_16(a + b))
    assert ids.summary_id(a, chunks) == ids.summary_id(a, list(reversed(chunks)))


# ------------------------------------------------------------------ validator subset
def test_validator_keywords():
    sch = {"type": "object", "required": ["a"], "additionalProperties": False,
           "properties": {"a": {"type": "integer", "minimum": 1, "maximum": 3},
                          "b": {"type": "array", "items": {"type": "string", "minLength": 2}, "minItems": 1,
                                "uniqueItems": True},
                          "c": {"enum": ["x", "y"]}, "d": {"type": ["string", "null"], "format": "date-time"},
                          "e": {"oneOf": [{"type": "integer"}, {"type": "string"}]},
                          "f": {"anyOf": [{"const": 1}, {"const": 2}]},
                          "g": {"type": "string", "pattern": "^[0-9a-f]+$", "maxLength": 4}}}
    ok, errs = validate_json({"a": 2, "b": ["xx"], "c": "x", "d": None, "e": 3, "f": 2, "g": "ab"}, sch)
    assert ok, errs
    for bad in ({"a": 0}, {"a": 4}, {"a": "2"}, {"b": []}, {"a": 1, "b": ["x"]}, {"a": 1, "b": ["xx", "xx"]},
                {"a": 1, "c": "z"}, {"a": 1, "d": "yesterday"}, {"a": 1, "e": 1.5}, {"a": 1, "f": 3},
                {"a": 1, "g": "XYZ"}, {"a": 1, "g": "abcde"}, {"a": 1, "zz": 0}, {}):
        assert not validate_json(bad, sch)[0], bad
    assert not validate_json(True, {"type": "integer"})[0]  # bool is not an integer
    with pytest.raises(ValidationError):
        validate_or_raise({"a": 0}, sch)


def test_validator_refs():
    reg = SchemaRegistry()
    reg.add({"$id": "https://x/defs.json", "$defs": {"pos": {"type": "integer", "minimum": 0}}}, "defs.json")
    sch = {"type": "object", "properties": {"n": {"$ref": "defs.json#/$defs/pos"}},
           "$defs": {"name": {"type": "string"}}, "required": ["n"]}
    assert iter_errors({"n": 1}, sch, reg) == []
    assert iter_errors({"n": -1}, sch, reg)
    local = {"$defs": {"s": {"type": "string"}}, "properties": {"x": {"$ref": "#/$defs/s"}}}
    assert iter_errors({"x": "a"}, local) == []
    assert iter_errors({"x": 1}, local)
